"""bean_hip_survival_members_supported without a GPU: declared, exported by every build, listed where the ctypes layer
looks, and a null handle is an error that names the entry point."""
import os
import re

import pytest

import bean_amd  # noqa: F401
from bean_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bean_hip_survival_members_supported"


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_the_predicate_is_declared_listed_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "bean_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const\s+bean_hip_ctx\s*\*\s*ctx\s*\)\s*;", code)
    assert header.count(NAME) > code.count(NAME)  # and documented
    (entry,) = [s for s in _lib.SYMBOLS if s[0] == NAME]
    assert entry[1] is _lib.c_int32 and entry[2] == [_lib.c_void_p]
    assert NAME in _lib.ENSEMBLE_SYMBOLS  # an older build named by BEAN_HIP_LIB may lack it
    assert hasattr(lib, NAME)
    for amax in _lib.ALL_BUILDS:
        if os.path.exists(_lib.lib_path(amax)):
            assert hasattr(_lib.load(amax), NAME), amax


def test_a_null_handle_is_refused_with_the_name(lib):
    assert lib.bean_hip_survival_members_supported(None) < 0
    assert lib.bean_hip_last_error().decode() == NAME + ": null handle"
    assert lib.bean_hip_ensemble_supported(None) < 0  # (its neighbour's sentence is its own)
    assert lib.bean_hip_last_error().decode() == "bean_hip_ensemble_supported: null handle"


def test_the_run_layer_opts_in_by_name():
    """Survival plans are batched only where the caller asks: the default of the opt-in is off."""
    import inspect

    from bean_amd.model import run

    for fn in (run._fit_plan, run._fit_members):
        assert inspect.signature(fn).parameters["batch_survival"].default is False
