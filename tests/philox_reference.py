"""Host replay of the device's random draws from their Philox counters (numpy, float64, vectorised).

The generator is counter based, so the draw an engine exports at ``(seed, site, element, step)`` can be recomputed here
from those four numbers alone, with no knowledge of the launch.  Written from the published algorithms and from the key
layout that the comments of ``csrc/bean_special.hpp`` document:

* Philox4x32-10 (Salmon et al. 2011, Random123): ``philox4x32_10``; the known-answer vectors are in
  ``test_philox_reference.py``.
* rocRAND's keying: subsequence and offset select the counter, the seed is the key (``block``).
* rocRAND's ``box_muller(x, y)``: ``u = 2^-32 + x 2^-32``, ``v = 2 pi 2^-32 + y 2 pi 2^-32`` in float32, the pair
  ``(sin v, cos v) sqrt(-2 log u)`` (``rocrand_normal2``; evaluated in float64 here).
* Marsaglia & Tsang (2000) with the ``U^(1/alpha)`` boost for shapes below 1, two components per rejection loop on one
  running generator (``gamma_pair``), and the Dirichlet draws built on it (``dirichlet_pair``, ``dirichlet_A``).

Layout (``site`` in bits 48+ of the subsequence, the element below it; offsets count 32-bit words):

    site 1 target   element t_off + t                     offset 4 step     .x eps_mu, .y eps_sd
    site 2 pi       element r G_tot + g_off + g           offset 256 step   (wide tiling: times stride(A), + allele)
    site 3 noise    element g_off + g (or the stream id)  offset 4 step     .x
    site 4 aux      element g_off + g                     offset 4 step     .x  (survival: mu_negctrl)
    site 5 q0       element r0 G_tot + g_off + g, r0 even offset 256 step   replicates (r0, r0 + 1) share a loop
    site 6 cov      element i                             offset 4 step     .x

A pi or q0 element owns the 256 words (64 blocks) of its step: a draw that read more would run into the next step's.
``gamma_pair`` returns the generator position so that the tests can hold every replayed draw to that window.
"""
import numpy as np

SITE_TARGET, SITE_PI, SITE_NOISE, SITE_AUX, SITE_Q0, SITE_COV = 1, 2, 3, 4, 5, 6
M32 = np.uint64(0xFFFFFFFF)
DBL_MIN = float(np.finfo(np.float64).tiny)
ONE_MINUS = float(np.nextafter(1.0, 0.0))
FLT_MIN = float(np.finfo(np.float32).tiny)
TWO_M32 = 2.0 ** -32
MAX_ROUNDS = 64
# the floor shortcuts of bean_special.hpp: a boosted component whose U^(1/alpha) is below the threshold is on its
# caller's floor whatever the rejection loop would give, and skips it (1: FLT_MIN / 128, 2: DBL_MIN / 2e3);
# the float32 pre-test is log U < kLogFloor alpha - 1e-5
SCALE_FLOOR = {1: 9.18e-41, 2: 1e-311}
LOG_FLOOR = {1: -92.5, 2: -716.5}


def _u64(v):
    if isinstance(v, (int, np.integer)):
        return np.uint64(int(v) & 0xFFFFFFFFFFFFFFFF)
    return np.asarray(v).astype(np.uint64)


def philox4x32_10(counter4, key2):
    """Ten rounds of Philox4x32.  ``counter4``: four arrays (or ints) of 32-bit words, ``key2``: two.  Returns the
    four output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (_u64(c) & M32 for c in counter4)
    k0, k1 = (_u64(k) & M32 for k in key2)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & M32, (p0 >> s32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return c0, c1, c2, c3


def block(seed, sub, offset):
    """The block (x, y, z, w) of a rocRAND Philox state ``rocrand_init(seed, sub, offset)``, ``offset`` a multiple of
    four words: counter ``(offset >> 2, sub)`` in 32-bit halves, low first; key the halves of ``seed``."""
    seed, sub, offset = _u64(seed), _u64(sub), _u64(offset)
    blk = offset >> np.uint64(2)
    s32 = np.uint64(32)
    return philox4x32_10((blk & M32, blk >> s32, sub & M32, sub >> s32), (seed & M32, seed >> s32))


def subsequence(site, element):
    return (np.uint64(site) << np.uint64(48)) + _u64(element)


def to_unit(a, b):
    """(0, 1] from the top 53 bits of ``(a << 32) | b``."""
    bits = ((_u64(a) << np.uint64(32)) | _u64(b)) >> np.uint64(11)
    return (bits.astype(np.float64) + 1.0) * 2.0 ** -53


def rocrand_normal2(x, y):
    """rocRAND's float32 Box-Muller of two words: the uniforms are formed in float32 as rocRAND forms them, the
    logarithm, root, sine and cosine in float64.  Returns ``(.x, .y, radius)``; ``.x`` is the sine branch."""
    fx = _u64(x).astype(np.float32)
    fy = _u64(y).astype(np.float32)
    u = (np.float32(TWO_M32) + fx * np.float32(TWO_M32)).astype(np.float64)  # float32 sum of an exact product
    c = np.float64(np.float32(1.46291807e-09))  # ROCRAND_2POW32_INV_2PI
    v = (c + fy.astype(np.float64) * c).astype(np.float32).astype(np.float64)  # one rounding: a fused multiply-add
    s = np.sqrt(-2.0 * np.log(u))
    return np.sin(v) * s, np.cos(v) * s, s


def normal_at(seed, site, element, step):
    """The float32 normals ``(.x, .y)`` and their radius at offset ``4 step`` of ``(site, element)``."""
    x, y, _, _ = block(seed, subsequence(site, element), _u64(step) * np.uint64(4))
    return rocrand_normal2(x, y)


def gamma_round(blk):
    """Random inputs of one rejection round for two components from one block: words x, y give two float32 Box-Muller
    normals (u1 = (x + 1) 2^-32 and u2 = y 2^-32 in float32; cosine first), words z, w two acceptance uniforms.
    Returns ``(na, nb, radius, ua, ub)``; the normals are rounded to float32."""
    x, y, z, w = blk
    u1 = ((_u64(x).astype(np.float32) + np.float32(1.0)) * np.float32(TWO_M32)).astype(np.float64)
    u2 = (_u64(y).astype(np.float32) * np.float32(TWO_M32)).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = np.pi * (2.0 * u2)
    na = (rad * np.cos(ang)).astype(np.float32).astype(np.float64)
    nb = (rad * np.sin(ang)).astype(np.float32).astype(np.float64)
    ua = (_u64(z).astype(np.float64) + 0.5) * TWO_M32
    ub = (_u64(w).astype(np.float64) + 0.5) * TWO_M32
    return na, nb, rad, ua, ub


def normal_bound(K, radius):
    """What a float32 Box-Muller normal of the device may differ by from this reference: K 2^-24 max(1, radius)."""
    return K * 2.0 ** -24 * np.maximum(1.0, radius)


SQUEEZE = 0.0331


def _decisions(n, u, d, c, squeeze=SQUEEZE):
    """One component's decisions in a round: (1 + c n > 0, the squeeze, the log test), and how close the float64
    arithmetic itself is to turning one of them."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        y = 1.0 + c * n
        pos = y > 0.0
        v = y * y * y
        xx = n * n
        bound = 1.0 - squeeze * xx * xx
        sq = pos & (u < bound)
        lu, lv = np.log(u), np.log(np.where(pos, v, 1.0))
        t = 0.5 * xx + d * (1.0 - v + lv) - lu
        lg = pos & (t > 0.0)
        near = (np.abs(y) < 1e-12) | (pos & (np.abs(u - bound) < 1e-14)) | (
            pos & ~sq & (np.abs(t) < 1e-12 * (1.0 + np.abs(lu) + d * (1.0 + np.abs(lv)))))
    return pos, sq, lg, near


def gamma_pair(a0, a1, seed, sub, offset, floor=0, K=0.0, squeeze=SQUEEZE, boost_block=True):
    """Two Gamma(a_i, 1) draws per element from one running generator at ``(seed, sub, offset)``.

    One block for the two boost uniforms when either shape is below 1 (``U^(1/a)`` from words (x, y) and (z, w) as
    53-bit uniforms; the component is then drawn at shape a + 1), then one block per round for both components, up to
    64 rounds.  A round is rejected when ``1 + c n <= 0``, accepted when ``u < 1 - 0.0331 n^4``, and otherwise
    decided by ``log u < n^2 / 2 + d (1 - v + log v)``.  ``floor`` 1 / 2: a boosted component whose factor is below
    ``SCALE_FLOOR[floor]`` takes no part in the rounds (0 stands for its value: its caller floors it), and when both
    are, no round is drawn.  A shape of exactly 0 has the factor 0.

    ``K``: the normals are good to ``normal_bound(K, radius)``; an element any of whose decisions changes under that
    perturbation - or whose floor test is within the float32 logarithm's error of its threshold - is ``undecided``.
    ``squeeze`` and ``boost_block`` exist so that a test can show that a changed constant or a dropped block is seen.

    Returns ``(g0, g1, k, undecided, tol0, tol1)``: the values (unfloored), the generator position after the draw in
    blocks, the flag, and each value's first-order sensitivity to the perturbation plus 1e-13 relative."""
    a = np.stack(np.broadcast_arrays(np.asarray(a0, np.float64), np.asarray(a1, np.float64))).copy()
    n_el = a.shape[1]
    sub = np.broadcast_to(_u64(sub), (n_el,))
    offset = np.broadcast_to(_u64(offset), (n_el,))
    k = np.zeros(n_el, np.int64)
    scale = np.ones((2, n_el))
    undecided = np.zeros(n_el, bool)
    done = np.zeros((2, n_el), bool)
    boosted = a < 1.0
    idx = np.nonzero(boosted[0] | boosted[1])[0]
    if idx.size:
        x, y, z, w = block(seed, sub[idx], offset[idx])
        if boost_block:
            k[idx] = 1
        for i, U in enumerate((to_unit(x, y), to_unit(z, w))):
            ai = a[i, idx]
            m = boosted[i, idx]
            with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
                lexp = np.where(ai > 0.0, np.log(U) / np.where(ai > 0.0, ai, 1.0), -np.inf)
                s = np.where(m, np.exp(lexp), 1.0)
            scale[i, idx] = s
            if floor:
                lf = np.log(SCALE_FLOOR[floor])
                done[i, idx] = m & (s < SCALE_FLOOR[floor])
                with np.errstate(invalid="ignore"):
                    # the float64 test within its own arithmetic of the threshold, or the float32 pre-test within a
                    # float32 logarithm's error of its threshold
                    close = np.abs(lexp - lf) < 1e-9 * np.abs(lf)
                    thr = LOG_FLOOR[floor] * ai - 1e-5
                    close |= np.abs(np.log(U) - thr) < 2.0 ** -20 * (1.0 + np.abs(thr))
                undecided[idx] |= m & close
    a = np.where(boosted, a + 1.0, a)
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    g = d.copy()  # what a component that 64 rounds did not settle keeps
    sens = np.zeros((2, n_el))
    for _ in range(MAX_ROUNDS):
        idx = np.nonzero(~(done[0] & done[1]))[0]
        if not idx.size:
            break
        na, nb, rad, ua, ub = gamma_round(block(seed, sub[idx], offset[idx] + np.uint64(4) * k[idx].astype(np.uint64)))
        k[idx] += 1
        dn = normal_bound(K, rad)
        for i, (n, u) in enumerate(((na, ua), (nb, ub))):
            live = ~done[i, idx]
            di, ci = d[i, idx], c[i, idx]
            pos, sq, lg, near = _decisions(n, u, di, ci, squeeze)
            und = near
            if K > 0.0:
                for nn in (n - dn, n + dn):
                    pos2, sq2, lg2, _ = _decisions(nn, u, di, ci, squeeze)
                    und = und | (pos2 != pos) | (sq2 != sq) | (~sq & ~sq2 & (lg2 != lg))
            undecided[idx] |= live & und
            new = live & pos & (sq | lg)
            j = idx[new]
            y = 1.0 + ci[new] * n[new]
            g[i, j] = di[new] * y * y * y
            sens[i, j] = di[new] * 3.0 * y * y * ci[new] * dn[new]
            done[i, j] = True
    val = np.where(scale < (SCALE_FLOOR[floor] if floor else 0.0), 0.0, scale * g)
    tol = scale * sens + 1e-13 * np.abs(val)
    return val[0], val[1], k, undecided, tol[0], tol[1]


def dirichlet_pair(a0, a1, seed, sub, offset, floor=0, K=0.0, **kw):
    """A two-component Dirichlet draw: the gammas floored at DBL_MIN, normalised, clamped to [DBL_MIN, 1 - eps].
    Returns ``(pi0, pi1, k, undecided, tol0, tol1)``."""
    g0, g1, k, und, t0, t1 = gamma_pair(a0, a1, seed, sub, offset, floor, K, **kw)
    g0, g1 = np.maximum(g0, DBL_MIN), np.maximum(g1, DBL_MIN)
    s = g0 + g1
    p0, p1 = np.clip(g0 / s, DBL_MIN, ONE_MINUS), np.clip(g1 / s, DBL_MIN, ONE_MINUS)
    tol = (p1 * t0 + p0 * t1) / s  # d p0 = (g1 d g0 - g0 d g1) / s^2
    return p0, p1, k, und, tol + 1e-13 * p0, tol + 1e-13 * p1


def dirichlet_A(conc, seed, sub, offset, floor=0, K=0.0, **kw):
    """An A-component Dirichlet draw per element (``conc``: (N, A)) on ONE running generator: components are drawn two
    at a time, each pair starting where the previous one stopped; an odd last component is paired with shape 1.0.
    Gammas floored at DBL_MIN, normalised, clamped.  Returns ``(pi (N, A), k, undecided, tol (N, A))``."""
    conc = np.asarray(conc, np.float64)
    n_el, A = conc.shape
    sub = np.broadcast_to(_u64(sub), (n_el,))
    offset = np.broadcast_to(_u64(offset), (n_el,))
    gam, tol = np.zeros((n_el, A)), np.zeros((n_el, A))
    k = np.zeros(n_el, np.int64)
    und = np.zeros(n_el, bool)
    for a in range(0, A, 2):
        second = conc[:, a + 1] if a + 1 < A else np.ones(n_el)
        g0, g1, kk, u, t0, t1 = gamma_pair(conc[:, a], second, seed, sub, offset + np.uint64(4) * k.astype(np.uint64),
                                           floor, K, **kw)
        k += kk
        und |= u
        gam[:, a], tol[:, a] = np.maximum(g0, DBL_MIN), t0
        if a + 1 < A:
            gam[:, a + 1], tol[:, a + 1] = np.maximum(g1, DBL_MIN), t1
    s = gam.sum(1, keepdims=True)
    pi = np.clip(gam / s, DBL_MIN, ONE_MINUS)
    return pi, k, und, (tol + pi * tol.sum(1, keepdims=True)) / s + 1e-13 * pi


# ---------------------------------------------------------------------------------------------------------------
# One function per site: the draws of a whole screen (or shard) at (seed, step).
# ---------------------------------------------------------------------------------------------------------------
def target_draws(seed, step, n_targets, t_off=0):
    """Site 1.  Element ``t_off + t`` for target (tiling: edit) ``t`` of the engine, offset ``4 step``; ``.x`` is
    eps_mu and ``.y`` eps_sd, exported in target order (``drawn_noise()`` reshapes them to (T, 1) for the variant
    families).  Returns ``(eps_mu, eps_sd, radius)``."""
    return normal_at(seed, SITE_TARGET, t_off + np.arange(n_targets), step)


def noise_draws(seed, step, n_guides, g_off=0, stream_ids=None):
    """Site 3 (accessibility noise).  Element ``g_off + g`` - or the guide's stream id, its index in the whole screen,
    where the engine holds its guides in another order (tiling with ``guide_ids``) -, offset ``4 step``, ``.x``;
    exported per guide in the caller's guide order.  Returns ``(eps_noise, radius)``."""
    el = g_off + np.arange(n_guides) if stream_ids is None else np.asarray(stream_ids)
    x, _, rad = normal_at(seed, SITE_NOISE, el, step)
    return x, rad


def aux_draws(seed, step, n_guides, g_off=0):
    """Site 4 (survival mixture: the per-guide baseline growth).  Element ``g_off + g``, offset ``4 step``, ``.x``;
    ``drawn_noise()`` exports ``mu_negctrl = m0 + eps s0`` with the float32 constants of the prior.  Returns
    ``(eps_u, radius)``."""
    x, _, rad = normal_at(seed, SITE_AUX, g_off + np.arange(n_guides), step)
    return x, rad


def cov_draws(seed, step, n_cov):
    """Site 6 (sample covariates of the sorting Normal model).  Element ``i`` for covariate ``i`` (replicated on every
    shard: no offset), offset ``4 step``, ``.x``; exported as ``eps_cov`` (n_cov,).  Returns ``(eps_cov, radius)``."""
    x, _, rad = normal_at(seed, SITE_COV, np.arange(n_cov), step)
    return x, rad


def pi_pair_screen(seed, step, conc, n_reps, G_tot=None, g_off=0, K=0.0, stride=256, **kw):
    """Site 2, two components (variant families).  Element ``r G_tot + g_off + g`` for replicate ``r`` and guide ``g``
    of the engine (``G_tot``: guides of the WHOLE screen, ``g_off``: this shard's first), offset ``256 step``, plain
    sampler (floor 0), both components on one generator.  ``conc`` (G, 2): the guide-side concentrations, the same for
    every replicate.  Exported as ``pi`` (R, 1, G, 2) whether or not ``repguide_mask`` masks the (replicate, guide): the
    mask acts on the likelihood.  Returns ``(pi (R, G, 2), k (R, G), undecided (R, G), tol (R, G, 2))``."""
    conc = np.asarray(conc, np.float64)
    G = conc.shape[0]
    G_tot = G if G_tot is None else G_tot
    el = (np.arange(n_reps)[:, None] * G_tot + g_off + np.arange(G)[None, :]).reshape(-1)
    a0, a1 = np.tile(conc[:, 0], n_reps), np.tile(conc[:, 1], n_reps)
    p0, p1, k, und, t0, t1 = dirichlet_pair(a0, a1, seed, subsequence(SITE_PI, el), _u64(step) * np.uint64(stride),
                                            0, K, **kw)
    sh = (n_reps, G)
    return np.stack([p0, p1], -1).reshape(sh + (2,)), k.reshape(sh), und.reshape(sh), np.stack([t0, t1], -1).reshape(
        sh + (2,))


def pi_tiling_screen(seed, step, conc, n_reps, G_tot=None, g_off=0, K=0.0, stream_ids=None):
    """Site 2, A <= 32 components (the register-resident tiling kernels).  Element ``r G_tot + id`` with ``id`` the
    guide's stream id (``g_off + g``, or its index in the whole screen under ``guide_ids``), offset ``256 step``; the
    components of a guide are drawn two at a time on that one generator (``dirichlet_A``, plain sampler).  ``conc``
    (G, A).  Exported as ``pi`` (R, 1, G, A); a (replicate, guide) that ``repguide_mask`` masks exports 1 / A in every
    component.  Returns ``(pi (R, G, A), k, undecided, tol)``."""
    conc = np.asarray(conc, np.float64)
    G, A = conc.shape
    G_tot = G if G_tot is None else G_tot
    ids = g_off + np.arange(G) if stream_ids is None else np.asarray(stream_ids)
    el = (np.arange(n_reps)[:, None] * G_tot + ids[None, :]).reshape(-1)
    pi, k, und, tol = dirichlet_A(np.tile(conc, (n_reps, 1)), seed, subsequence(SITE_PI, el),
                                  _u64(step) * np.uint64(256), 0, K)
    return pi.reshape(n_reps, G, A), k.reshape(n_reps, G), und.reshape(n_reps, G), tol.reshape(n_reps, G, A)


def wide_stream_stride(A):
    return 256 if A <= 256 else 1024


def pi_wide_screen(seed, step, conc, n_reps, G_tot=None, g_off=0, K=0.0, stream_ids=None):
    """Site 2, the allele-parallel (wide) tiling kernel, A > 32.  Alleles ``a`` and ``a + 64`` (``a`` modulo 128 below
    64) share one rejection loop on the generator of the first: element ``(r G_tot + id) stride(A) + a``, offset
    ``256 step``, the double-floor sampler (floor 2); an allele without a partner below A is paired with shape 1.0.
    Gammas floored at DBL_MIN, normalised over the guide, clamped.  Exported as ``pi`` (R, 1, G, A); masked
    (replicate, guide): 1 / A.  Returns ``(pi (R, G, A), k (R, G, A) - of each allele's generator -, undecided (R, G),
    tol)``."""
    conc = np.asarray(conc, np.float64)
    G, A = conc.shape
    G_tot = G if G_tot is None else G_tot
    ids = g_off + np.arange(G) if stream_ids is None else np.asarray(stream_ids)
    base = (np.arange(n_reps)[:, None] * G_tot + ids[None, :]).reshape(-1) * wide_stream_stride(A)
    N = base.size
    cc = np.tile(conc, (n_reps, 1))
    gam, tol, kk = np.zeros((N, A)), np.zeros((N, A)), np.zeros((N, A), np.int64)
    und = np.zeros(N, bool)
    for a in range(A):
        if (a % 128) >= 64:
            continue
        a2 = a + 64
        second = cc[:, a2] if a2 < A else np.ones(N)
        g0, g1, k, u, t0, t1 = gamma_pair(cc[:, a], second, seed, subsequence(SITE_PI, base + a),
                                          _u64(step) * np.uint64(256), 2, K)
        und |= u
        gam[:, a], tol[:, a], kk[:, a] = np.maximum(g0, DBL_MIN), t0, k
        if a2 < A:
            gam[:, a2], tol[:, a2], kk[:, a2] = np.maximum(g1, DBL_MIN), t1, k
    s = gam.sum(1, keepdims=True)
    pi = np.clip(gam / s, DBL_MIN, ONE_MINUS)
    tol = (tol + pi * tol.sum(1, keepdims=True)) / s + 1e-13 * pi
    return pi.reshape(n_reps, G, A), kk.reshape(n_reps, G, A), und.reshape(n_reps, G), tol.reshape(n_reps, G, A)


def q0_screen(seed, step, conc, n_reps, G_tot=None, g_off=0, K=0.0):
    """Site 5 (survival mixture: the Dirichlet over ALL guides).  Replicates ``(r0, r0 + 1)``, ``r0`` even, of guide
    ``g`` share one loop on element ``r0 G_tot + g_off + g``, offset ``256 step``, the float32-floor sampler (floor 1),
    both at the guide's concentration; an odd last replicate is paired with shape 0.  Each gamma is rounded to float32
    and floored at FLT_MIN.  The engine exports ``initial_abundance`` (R, G) = the gamma divided by its replicate's
    total over the whole screen, rounded to float32 and clamped to [FLT_MIN, 1 - 2^-24]; this returns the gammas
    ``(gamma (R, G), k (ceil(R / 2), G), undecided (R, G), tol (R, G))``."""
    conc = np.asarray(conc, np.float64)
    G = conc.size
    G_tot = G if G_tot is None else G_tot
    gam, tol = np.zeros((n_reps, G)), np.zeros((n_reps, G))
    und = np.zeros((n_reps, G), bool)
    ks = []
    for r0 in range(0, n_reps, 2):
        two = r0 + 1 < n_reps
        el = r0 * G_tot + g_off + np.arange(G)
        g0, g1, k, u, t0, t1 = gamma_pair(conc, conc if two else np.zeros(G), seed, subsequence(SITE_Q0, el),
                                          _u64(step) * np.uint64(256), 1, K)
        ks.append(k)
        f32 = lambda v: np.maximum(v.astype(np.float32), np.float32(FLT_MIN)).astype(np.float64)
        gam[r0], tol[r0], und[r0] = f32(g0), t0, u
        if two:
            gam[r0 + 1], tol[r0 + 1], und[r0 + 1] = f32(g1), t1, u
    return gam, np.stack(ks), und, tol


# ---------------------------------------------------------------------------------------------------------------
# What the GPU tests measured ("The draws replayed from their counters"): the worst
# |device - reference| / (2^-24 max(1, radius)) of a float32 Box-Muller normal, times four, rounded up to a power
# of two.  K_ROCRAND: rocRAND's form (fast sine and cosine); K_GAMMA: gamma_round's logf / sincospif.  At most 2^10.
# ---------------------------------------------------------------------------------------------------------------
K_ROCRAND = 32.0
K_GAMMA = 64.0


# the op-level cases that test_gpu_draw_replay.py runs and test_philox_reference.py measures the undecided shares of
OP_N = 1 << 16
OP_SEED = 0x9E3779B97F4A7C15
OP_SHAPE_PAIRS = [(0.3, 0.7), (0.9, 14.0), (2.5, 2.5), (40.0, 7.0), (10.7, 333.0), (1.0, float(np.nextafter(1.0, 0.0))),
                  (1e-5, 3.0), (1e-5, 1e-5), (2e-3, 1e-5), (0.05, 0.3), (5e-7, 1.0), (2.0, 1e-6)]
OP_EXPORT_PAIRS = [(0.3, 0.7), (10.7, 333.0), (1e-5, 3.0), (5e-7, 1.0)]


def op_case(site, a0, a1, floor, K=None):
    """The replay of one op-level case: OP_N elements, element i at (OP_SEED, site, i, offset 0)."""
    return gamma_pair(np.full(OP_N, a0), np.full(OP_N, a1), OP_SEED, subsequence(site, np.arange(OP_N)), 0, floor,
                      K_GAMMA if K is None else K)


def settled_log(target):
    """float32 parameters ``p`` next to ``log(target)`` whose exponential is settled in float32: ``exp(p)`` lies within
    0.02 float32 ulp of a float32 number, so every ``expf`` good to 0.98 ulp returns that number - the replay then knows
    the concentration the device forms from the parameter without knowing its ``expf``.  Returns ``(p, exp(p) as the
    float32 number, in float64)``.  Targets should be away from 1 (|log| > 0.5: nearer, the exponential moves by much
    less than an ulp per step of p and the search is long)."""
    p = np.log(np.asarray(target, np.float64)).astype(np.float32).reshape(-1)
    val = np.zeros(p.size)
    todo = np.ones(p.size, bool)
    for _ in range(20000):
        e = np.exp(p[todo].astype(np.float64))
        f = e.astype(np.float32)
        ok = np.abs(e - f.astype(np.float64)) < 0.02 * np.spacing(f).astype(np.float64)
        j = np.nonzero(todo)[0]
        val[j[ok]] = f[ok].astype(np.float64)
        todo[j[ok]] = False
        if not todo.any():
            break
        p[todo] = np.nextafter(p[todo], np.float32(np.inf))
    assert not todo.any()
    return p.reshape(np.shape(target)), val.reshape(np.shape(target))
