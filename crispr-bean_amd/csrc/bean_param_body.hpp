// The body of k_param<FINISH, ADAM, PREP, KIND> (bean_kernels.hpp) and of k_param_ens (bean_ensemble.hpp): NOT a header
// of its own - it is included INSIDE a kernel that has `DevArgs c`, `int n_target_blocks` and the four template
// parameters in scope.  Kept as text so that the single-fit kernel stays, token for token, what it was before the
// ensemble kernel existed (a shared __device__ function taking the arguments by reference compiled k_param differently:
// other register counts in every instantiation).
#ifndef BEAN_PARAM_BODY_INCLUDED_BY_KERNEL
#error "bean_param_body.hpp is the text of a kernel body: include it from inside k_param / k_param_ens only"
#endif
    // (KIND 3: what the grid holds beyond the edit blocks and the guide blocks - kAMax lanes per guide - are allele blocks)
    const int n_allele_blocks =
        KIND == 3 ? (int)gridDim.x - n_target_blocks - (int)(((long)c.G * kAMax + kParamBlock - 1) / kParamBlock) : 0;
    if (KIND == 1) {
        __builtin_assume(c.lpt == kLanesPerTarget);
        __builtin_assume(!c.survival);
        __builtin_assume(c.family != kMultiMixture);
        __builtin_assume(!c.wide_targets);
        __builtin_assume(c.tgrad == nullptr);
        __builtin_assume(c.n_cov == 0);
        __builtin_assume(c.wrow != nullptr);
        __builtin_assume(c.rows_v2 != 0);
        __builtin_assume(c.rrow == nullptr);
        __builtin_assume(!c.surv_q0lik);
        __builtin_assume(!c.not_loss_owner);
        __builtin_assume(c.lpart != nullptr);
        __builtin_assume(c.dgq != nullptr || c.family != kMixture);
        __builtin_assume(c.tsum != nullptr);
    }
    if (KIND == 2) {  // survival variant MixtureNormal on the wave-form path (thin mode, unsharded parameters)
        __builtin_assume(c.lpt == kLanesPerTargetNarrow);
        __builtin_assume(c.survival != 0);
        __builtin_assume(c.family == kMixture);
        __builtin_assume(!c.surv_q0lik);
        __builtin_assume(c.dgq != nullptr);
        __builtin_assume(c.tsum == nullptr);
        __builtin_assume(!c.wide_targets);
        __builtin_assume(c.tgrad == nullptr);
        __builtin_assume(c.n_cov == 0);
        __builtin_assume(c.wrow != nullptr);
        __builtin_assume(c.rows_v2 != 0);
        __builtin_assume(c.rrow == nullptr);
        __builtin_assume(c.lpart != nullptr);
    }
    if (KIND == 3) {  // tiling (MultiMixtureNormal) in the register-resident wave form, thin mode
        __builtin_assume(c.lpt == kLanesPerTargetNarrow);
        __builtin_assume(c.family == kMultiMixture);
        __builtin_assume(!c.wide_targets);
        __builtin_assume(!c.wide_alleles);
        // (c.tgrad: either - a guide-sharded fit's exchanged update is this build too, with its allele blocks)
        __builtin_assume(c.n_cov == 0);
        __builtin_assume(c.lpart == nullptr);
        __builtin_assume(c.trow_summed != 0);
        __builtin_assume(!c.surv_q0lik);
    }
    // (dispatch order: edit blocks, c.q0_blk0 guide blocks, the allele blocks, the other guide blocks - launch_param)
    const int allele_blk0 = n_target_blocks + c.q0_blk0;
    if (KIND == 3 && PREP && n_allele_blocks > 0 && (int)blockIdx.x >= allele_blk0 &&
        (int)blockIdx.x < allele_blk0 + n_allele_blocks) {
        const long idx = (long)((int)blockIdx.x - allele_blk0) * blockDim.x + threadIdx.x;
        const int stamp_rec = (int)gridDim.x - n_allele_blocks + ((int)blockIdx.x - allele_blk0);  // behind the guide blocks' records
        (void)stamp_rec;
        BEAN_STAMP_RT(stamp_rec, 0);
        const bool in = idx < c.n_live_slots;
        const int sl = in ? c.live_slots[idx] : 0;  // a1 * G + g
        {
            // data the slot's chain begins with, asked for now (the loads behind the poll then find it in the caches)
            const int a1 = sl / c.G, g = sl - a1 * c.G;
            const long slot = (long)g * (c.A - 1) + a1;
            const int k0 = c.a2e_ptr[slot], k1 = c.a2e_ptr[slot + 1];
            const int e0 = k0 < k1 ? c.a2e_idx[k0] : 0;
            const int am = c.amask[(long)g * c.A + a1 + 1];
            asm volatile("" ::"v"(e0), "v"(am), "v"(k1));
        }
        if (threadIdx.x == 0) {
            const int* const go = c.tile_ctr + 32 * (2 + ((int)blockIdx.x & (kAlleleGoFlags - 1)));
            int spins = 0;
            while (__hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
                if (++spins > kAlleleSpinMax) {
                    const StepCtr cs = *c.ctrA;
                    atomicAdd((unsigned long long*)(c.loss_acc + ((long)cs.slot * kLossSub) * kLossWords) + 2, 1ull);
                    break;
                }
                __builtin_amdgcn_s_sleep(16);
            }
        }
        __syncthreads();
        asm volatile("" ::: "memory");  // (nothing below is loaded before the poll has matched)
        BEAN_STAMP_RT(stamp_rec, 1);
        if (in) allele_slot_tables<2>(c, sl / c.G, sl % c.G);
        __syncthreads();
        BEAN_STAMP_RT(stamp_rec, 7);
        if (threadIdx.x == 0) {
            const int old = __hip_atomic_fetch_add(c.tile_ctr + 32, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old == n_allele_blocks - 1) {
                for (int k = 0; k < kAlleleCtrLines; ++k)
                    __hip_atomic_store(c.tile_ctr + 32 * k, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        return;
    }
    // Block roles, in role order: target blocks, guide blocks, (survival q0 site) q0 blocks.  The q0
    // blocks hold the kernel's longest chain (parameter update -> gamma draws -> block sums -> the last
    // one's totals, ~15 us at BASELINE config 5 against ~10 us of an alpha_pi guide block and ~5 us of a
    // target block), so they are dispatched first, the guide blocks next and the target blocks last.
    // (As a tail of the guide blocks - this round's first form - the draws began when the alpha_pi update
    // ended: k_param 33 us.  As blocks of their own that waited for a guide block's flag: 35 us.  Without a
    // q0 site the order of guide and target blocks makes no difference: measured on configs 1 and 3.)
    unsigned bid = blockIdx.x;
    if (KIND == 3 && PREP && n_allele_blocks > 0 && (int)blockIdx.x >= allele_blk0) bid -= (unsigned)n_allele_blocks;
    if (c.q0_blocks) {
        const unsigned ntb = (unsigned)n_target_blocks, nq0 = (unsigned)c.n_gamma_blocks, ngd = (unsigned)c.q0_blk0;
        if (blockIdx.x < nq0) bid = ntb + ngd + blockIdx.x;
        else if (blockIdx.x < nq0 + ngd) bid = ntb + (blockIdx.x - nq0);
        else bid = blockIdx.x - nq0 - ngd;
    }
    __shared__ double scratch[16];
    __shared__ double hand[4][kTargetsPerBlockMax];  // phase hand-over: gmu, gy (A -> B), mu, y (B -> C)
#if BEAN_KP_DIAG == 1  // diagnostic builds (wrong results): time the target part alone ...
    if ((int)bid >= n_target_blocks) return;
#elif BEAN_KP_DIAG == 2  // ... or the guide part alone
    if ((int)bid < n_target_blocks && bid != 0) return;
#endif
#if defined(BEAN_STAMP) && BEAN_STAMP == 2
    const int lane = threadIdx.x & 63;
    const long wave_gid = (long)bid * (kParamBlock / 64) + (threadIdx.x >> 6);
#endif
    BEAN_STAMP_KP(0);
    if (PREP && FINISH) BEAN_STAMP_RT(bid, 0);
    const StepCtr ctr = *c.ctrA;
    const unsigned long long s_prep = FINISH ? ctr.step + 1 : ctr.step;
    const unsigned long long slot_prep = FINISH ? ctr.slot + 1 : ctr.slot;
    AdamCoef ak;
    ak.step_size = 0.f;
    ak.clip = 0.f;
    if (FINISH && ADAM) {
        ak.step_size = ctr.step_size;  // of update t = ctr.step + 1, computed by the guide kernel (publish_ctr)
        ak.clip = (float)c.clip;
    }
    double loss_fin = 0.0, loss_prep = 0.0;
    const bool mixture = c.family == kMixture;
    // The guide kernel's per-wave loss parts (wave_loss_out).  Thin mode: every target block takes its
    // share; the block's LAST wave issues the loads now and adds them up while it would otherwise idle at
    // the barrier behind phase B (summed by the first blocks at the end of the kernel, they were the last
    // ~2 us of its critical path).  Other modes: the strided pass at the end.
    __shared__ long long lp3[3];
    const bool lp_early = FINISH && c.lpart != nullptr && !c.wide_targets && !c.tgrad;
    long long lw0 = 0, lw1 = 0, lw2 = 0;
    if (lp_early && (int)bid < n_target_blocks && threadIdx.x >= blockDim.x - 64) {
        const long per = (c.n_lpart + n_target_blocks - 1) / n_target_blocks;
        const long e0 = (long)bid * per, e1 = e0 + per < c.n_lpart ? e0 + per : c.n_lpart;
        for (long i = e0 + (threadIdx.x & 63); i < e1; i += 64) {
            lw0 += c.lpart[3 * i];
            lw1 += c.lpart[3 * i + 1];
            lw2 += c.lpart[3 * i + 2];
        }
    }

    if (c.survival && mixture && (int)bid >= n_target_blocks + c.q0_blk0) {
        // survival MixtureNormal: the Dirichlet(q0) site over ALL guides and the per-guide
        // baseline growth draw (survival_model.py:259-274,306-311,660-669)
        const int gb = (int)bid - n_target_blocks - c.q0_blk0;
        const int g = gb * kParamBlock + threadIdx.x;
        const bool in = g < c.G;
        float q0u = in ? c.p[7][g] : 0.f;
        if (FINISH && in) {
            float q0m = 0.f, q0v = 0.f;
            if (ADAM) {
                q0m = c.m[7][g];
                q0v = c.v[7][g];
            }
            const double q0 = (double)expf(q0u);
            emit_grad_pre<ADAM>(c, 7, g, part_row(c, kPQ0, g) * q0, ak, q0u, q0m, q0v);
            // - log p(mu_negctrl): Normal(m0, s0) built from Python floats => float32 tensors
            const float s0f = (float)c.neg_scale;
            const double du = c.u_g[g] - (double)(float)c.neg_loc;
            loss_fin += du * du / (2.0 * (double)(s0f * s0f)) + (double)logf(s0f) + kHalfLog2PiC;
        }
        if (PREP) {
            double q0 = 0.0;
            if (in) {
                q0 = (double)expf(q0u);
                double eps;
                if (c.eps_u_in) {
                    eps = c.eps_u_in[g];
                } else {
                    eps = (double)normal2_at(c.seed, ((unsigned long long)kSiteAux << 48) + (unsigned long long)(c.g_off + g),
                                                 s_prep * 4ull).x;
                }
                c.eps_u[g] = eps;
                c.u_g[g] = (double)(float)c.neg_loc + eps * (double)(float)c.neg_scale;
                if (c.eps_u_out) c.eps_u_out[g] = eps;
            }
            q0_draws_and_totals(c, gb, g, in, q0, s_prep, bid);
        }
    }
    if ((int)bid < n_target_blocks) {
        // ------------------------------------------------ target part
        // (the edit blocks head the launch's longest chain when allele blocks follow; a raised issue priority for them -
        // s_setprio 2 - measured nothing: 142.1 against 142.1 us per step)
        int t;
        bool active;
        double gmu = 0.0, gy = 0.0, tab_mu = 0.0, tab_y = 0.0;
        target_of_thread(c, t, active, bid);
        // sorting families: the target's parameters, moments and last draw are loaded BEFORE the
        // gradient sums (independent of them), not after
        float pf[4] = {0.f, 0.f, 0.f, 0.f}, mf[4] = {0.f, 0.f, 0.f, 0.f}, vf[4] = {0.f, 0.f, 0.f, 0.f};
        double eps1_f = 0.0, eps2_f = 0.0, mu_f = 0.0, y_f = 0.0;
        if (active) {
            const int n_lat = c.survival ? 2 : 4;  // survival: mu only (loc, scale)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < n_lat) {
                    pf[i] = c.p[i][t];
                    if (FINISH && ADAM) {
                        mf[i] = c.m[i][t];
                        vf[i] = c.v[i][t];
                    }
                }
            }
            if (FINISH) {
                eps1_f = c.eps_mu[t];
                mu_f = c.mu_t[t];
                if (!c.survival) {
                    eps2_f = c.eps_sd[t];
                    y_f = c.y_t[t];
                }
            }
        }
        // the standard normals of the NEXT step's draw depend on (seed, target, step) only: formed here, under
        // the latency of the loads above and of the gradient sums below, not behind the update they will be
        // scaled by (Philox + Box-Muller are ~250 instructions of this kernel's one-lane-per-target chain)
        float2 nrm_next = make_float2(0.f, 0.f);
        if (PREP && active && !c.eps_mu_in) {
            nrm_next = normal2_at(c.seed, ((unsigned long long)kSiteTarget << 48) + (unsigned long long)(c.t_off + t),
                                  s_prep * 4ull);
        }
        if (FINISH) {
            if (c.tgrad) {
                // sharded run of a family whose per-target parameters are shared across shards: the
                // sums were formed by k_target_reduce and all-reduced by the host
                if (active) {
                    gmu = c.tgrad[t];
                    gy = c.tgrad[c.T + t];
                }
            } else if (c.wide_targets) {
                target_grad_sums(c, t, active, scratch, gmu, gy);
            } else {
                // phase A (group map) -> phase B (owner map) through LDS
                int tg;
                bool lead;
                target_of_group(c, tg, lead, bid);
                double a, b;
                target_grad_sums(c, tg, lead, scratch, a, b);
                if (lead) {
                    hand[0][threadIdx.x / c.lpt] = a;
                    hand[1][threadIdx.x / c.lpt] = b;
                }
                __syncthreads();
                if (active) {
                    gmu = hand[0][threadIdx.x];
                    gy = hand[1][threadIdx.x];
                }
                if (lp_early && threadIdx.x >= blockDim.x - 64) {  // idle until the next barrier
                    lw0 = wave_sum_i64(lw0);
                    lw1 = wave_sum_i64(lw1);
                    lw2 = wave_sum_i64(lw2);
                    if ((threadIdx.x & 63) == 0) {
                        lp3[0] = lw0;
                        lp3[1] = lw1;
                        lp3[2] = lw2;
                    }
                }
            }
        }
        BEAN_STAMP_KP(1);
        if (active && c.survival) {
            // survival families: mu only (no sd latent), growth tables are computed in k_guide_survival
            // (parameters, moments and last draw loaded before the gradient sums, like the sorting families')
            float pl = pf[0], psu = pf[1];
            if (FINISH) {
                const double eps1 = eps1_f, mu = mu_f;
                const double s_mu = exp((double)psu);
                double logp_mu, dlogp_mu;
                if (c.flags & kPriorNormalMu) {
                    const double ploc = c.pr_mu_loc ? c.pr_mu_loc[t] : 0.0;
                    const double ps = c.pr_mu_scale ? c.pr_mu_scale[t] : 1.0;
                    const double zz = (mu - ploc) / ps;
                    logp_mu = -0.5 * zz * zz - log(ps) - kHalfLog2PiC;
                    dlogp_mu = -zz / ps;
                } else {
                    logp_mu = -kLog2 - fabs(mu);
                    dlogp_mu = mu > 0.0 ? -1.0 : (mu < 0.0 ? 1.0 : 0.0);
                }
                const double logq_mu = -0.5 * eps1 * eps1 - (double)psu - kHalfLog2PiC;
                loss_fin = -logp_mu + logq_mu;
                const double Gmu = gmu - dlogp_mu;
                emit_grad_pre<ADAM>(c, 0, t, Gmu, ak, pl, mf[0], vf[0]);
                emit_grad_pre<ADAM>(c, 1, t, Gmu * eps1 * s_mu - 1.0, ak, psu, mf[1], vf[1]);
            }
            if (PREP) {
                double eps1;
                if (c.eps_mu_in) {
                    eps1 = c.eps_mu_in[t];
                } else {
                    eps1 = (double)nrm_next.x;
                }
                c.eps_mu[t] = eps1;
                c.mu_t[t] = (double)pl + eps1 * exp((double)psu);
                if (c.eps_mu_out) c.eps_mu_out[t] = eps1;
            }
        } else if (active) {
            if (FINISH) {
                const double eps1 = eps1_f, eps2 = eps2_f;
                const double s_mu = exp((double)pf[1]), s_sd = exp((double)pf[3]);
                double dlogp_mu, dlogp_dy;
                tgt_prior_terms(c, t, tgt_sd_prior(c, t), mu_f, y_f, eps1, eps2, pf[1], pf[3], dlogp_mu, dlogp_dy,
                                loss_fin);
                const double Gmu = gmu - dlogp_mu;
                const double Gy = gy - dlogp_dy;
                emit_grad_pre<ADAM>(c, 0, t, tgt_grad(0, Gmu, eps1, s_mu), ak, pf[0], mf[0], vf[0]);
                emit_grad_pre<ADAM>(c, 1, t, tgt_grad(1, Gmu, eps1, s_mu), ak, pf[1], mf[1], vf[1]);
                emit_grad_pre<ADAM>(c, 2, t, tgt_grad(2, Gy, eps2, s_sd), ak, pf[2], mf[2], vf[2]);
                emit_grad_pre<ADAM>(c, 3, t, tgt_grad(3, Gy, eps2, s_sd), ak, pf[3], mf[3], vf[3]);
            }
            BEAN_STAMP_KP(2);
            if (PREP) {
                double eps1, eps2;
                if (c.eps_mu_in) {
                    eps1 = c.eps_mu_in[t];
                    eps2 = c.eps_sd_in[t];
                } else {
                    eps1 = (double)nrm_next.x;
                    eps2 = (double)nrm_next.y;
                }
                const double mu = tgt_draw(pf[0], eps1, pf[1]);
                const double y = tgt_draw(pf[2], eps2, pf[3]);
                c.eps_mu[t] = eps1;
                c.eps_sd[t] = eps2;
                // (KIND 3: written through - the allele blocks of this launch read them from other CUs)
                coh_st<KIND == 3 ? 2 : 0>(c.mu_t + t, mu);
                coh_st<KIND == 3 ? 2 : 0>(c.y_t + t, y);
                if (c.eps_mu_out) {
                    c.eps_mu_out[t] = eps1;
                    c.eps_sd_out[t] = eps2;
                }
                tab_mu = mu;
                tab_y = y;
            }
        }
        BEAN_STAMP_KP(3);
        // ---- Phi tables: the B entries of a target are spread over the lanes of its group
        // (thin mode: kLanesPerTarget consecutive lanes; wide mode: the block's first threads)
        if (PREP && !c.survival && c.family != kMultiMixture) {
            if (c.wide_targets) {
                if (threadIdx.x == 0) {
                    scratch[0] = tab_mu;
                    scratch[1] = tab_y;
                }
                __syncthreads();
                if ((int)threadIdx.x < c.B) {
                    if (c.n_cov)
                        for (int r = 0; r < c.R; ++r)
                            write_phi_entry(c, t, threadIdx.x, scratch[0] + c.cov_shift[r], scratch[1], (long)r * c.B * c.T);
                    else
                        write_phi_entry(c, t, threadIdx.x, scratch[0], scratch[1]);
                }
                __syncthreads();
            } else {
                // one lane per bin EDGE: even lane = upper edge, odd lane = lower edge of bin e >> 1, so
                // the erf / exp chain of a target is one edge deep (it was 2 B / 4 edges deep with four
                // lanes per target); the pair is combined with one shuffle.  Same formulas, same bits as
                // write_phi_entry.
                if (active) {
                    hand[2][threadIdx.x] = tab_mu;
                    hand[3][threadIdx.x] = tab_y;
                }
                __syncthreads();
                const int grp = threadIdx.x / kLanesPerTarget;
                t = (bid * blockDim.x + threadIdx.x) / kLanesPerTarget;  // group map from here on
                const double mu = hand[2][grp], y = hand[3][grp];
                const int j = threadIdx.x & (kLanesPerTarget - 1);
                const double sigma = c.family == kNormal ? exp(0.5 * y) : exp(y);
                const double dsig_dy = c.family == kNormal ? 0.5 * sigma : sigma;
                const double inv = 1.0 / sigma;
                const int n_tab = c.n_cov ? c.R : 1;  // sample covariates: one table per replicate
                for (int rt = 0; rt < n_tab; ++rt) {
                    const double mu_r = c.n_cov ? mu + c.cov_shift[rt] : mu;
                    const long off = (long)rt * c.B * c.T;
                    for (int e0 = 0; e0 < 2 * c.B; e0 += kLanesPerTarget)
                        phi_edge(c, t, t < c.T, e0 + j, mu_r, inv, dsig_dy, off);
                }
            }
        }
        BEAN_STAMP_KP(4);
        if (KIND == 3 && PREP && n_allele_blocks > 0) {
            // this edit block's draws are out: count in for the allele blocks
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (threadIdx.x == 0) {
                const int old = __hip_atomic_fetch_add(c.tile_ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (old == n_target_blocks - 1)  // the last edit block: every draw is out
                    for (int k = 0; k < kAlleleGoFlags; ++k)
                        __hip_atomic_store(c.tile_ctr + 32 * (2 + k), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            BEAN_STAMP_RT(bid, 4);
        }
    } else if (c.family == kMultiMixture) {
        const int guide_block = (int)bid - n_target_blocks;
        if (c.wide_alleles) param_guide_tiling_wide<FINISH, ADAM, PREP>(c, guide_block, s_prep, ak, loss_fin);
        else param_guide_tiling<FINISH, ADAM, PREP>(c, guide_block, s_prep, ak, loss_fin);
        if (c.survival) {
            // per-guide baseline growth mu_negctrl ~ N(m0, s0): sampled in the model only
            // (survival_model.py:479-483), i.e. a fresh prior draw each step
            const int tid = ((int)bid - n_target_blocks) * blockDim.x + threadIdx.x;
            // kAMax lanes per guide (param_guide_tiling) or one wave per guide (wide path): lane 0 acts
            const int lpg = c.wide_alleles ? 64 : kAMax;
            const int g = tid / lpg;
            if (g < c.G && tid % lpg == 0) {
                if (FINISH) {
                    const float s0f = (float)c.neg_scale;
                    const double du = c.u_g[g] - (double)(float)c.neg_loc;
                    loss_fin += du * du / (2.0 * (double)(s0f * s0f)) + (double)logf(s0f) + kHalfLog2PiC;
                }
                if (PREP) {
                    double eps;
                    if (c.eps_u_in) {
                        eps = c.eps_u_in[g];
                    } else {
                        eps = (double)normal2_at(c.seed, ((unsigned long long)kSiteAux << 48) + (unsigned long long)(c.g_off + g),
                                         s_prep * 4ull).x;
                    }
                    c.eps_u[g] = eps;
                    c.u_g[g] = (double)(float)c.neg_loc + eps * (double)(float)c.neg_scale;
                    if (c.eps_u_out) c.eps_u_out[g] = eps;
                }
            }
        }
    } else if (mixture) {
        // ------------------------------------------------- guide part
        // (survival: the q0 blocks follow the alpha_pi blocks; their g is out of range here)
        const int g = ((int)bid - n_target_blocks) * (int)blockDim.x + threadIdx.x;
        if (g < c.G) param_guide_mix<FINISH, ADAM, PREP, false>(c, g, ak, s_prep, loss_fin);
    }
    if (c.surv_q0lik && (int)bid >= n_target_blocks) {
        // survival NormalModel: Dirichlet(initial_abundance) site over ALL guides, drawn per
        // replicate and used by the likelihood (survival_model.py:62-67, 629-639).  The prior is
        // Dirichlet(1 / G), so unlike the MixtureNormal q0 site nothing cancels.
        const int gb = (int)bid - n_target_blocks;
        const int g = gb * kParamBlock + threadIdx.x;
        const bool in = g < c.G;
        float iau = in ? c.p[7][g] : 0.f;
        if (FINISH && in) {
            const double ia = (double)expf(iau);
            const double tot = c.gsum[c.R];
            double lg_tot, dg_tot, lg_a, dg_a;
            lgamma_digamma(tot, lg_tot, dg_tot);
            lgamma_digamma(ia, lg_a, dg_a);
            const double Rf = (double)c.R;
            // d/d ia of log q: direct term R (psi(tot) - psi(ia)) + sum_r log x, and the pathwise term
            double grad = Rf * (dg_tot - dg_a) + part_row(c, kPQ0, g);
            for (int r = 0; r < c.R; ++r) {
                const double gm = c.gam[(long)r * c.G + g];
                const double x = c.x0_in ? gm
                                         : (double)fminf(fmaxf((float)(gm * frcp(c.gsum[r])), 1.17549435e-38f),
                                                         0.99999994f);
                grad += dirichlet_grad_one(x, ia, tot) * (c.gq[(long)r * c.G + g] - c.sq[r]);
            }
            emit_grad<ADAM>(c, 7, g, grad * ia, ak);
            if (ADAM) iau = c.p[7][g];
            // normalisers: + log q: R (lgamma(tot) - sum lgamma(ia)); - log p: the prior
            // concentration is the float32 value of 1 / G on every guide (torch.ones(G) / G)
            const double pr = c.prior_ia ? c.prior_ia[g] : (double)(1.0f / (float)c.G_tot);
            double lg_p, dg_p;
            lgamma_digamma(pr, lg_p, dg_p);
            loss_fin += Rf * (lg_p - lg_a);
            if (c.g_off + g == 0) {  // once per screen (guide 0 of the whole screen)
                double lg_ps, dg_ps;
                lgamma_digamma(c.prior_ia ? c.prior_ia_total : pr * (double)c.G_tot, lg_ps, dg_ps);
                loss_fin += Rf * (lg_tot - lg_ps);
            }
        }
        if (PREP) {
            q0_draws_and_totals(c, gb, g, in, in ? (double)expf(iau) : 0.0, s_prep, bid);
        }
    }
    if (FINISH) {
        // replicated per-target parameters (sharded ControlNormal / tiling): their prior and entropy
        // terms are counted by one rank only
        // (sorting NormalModel with sample covariates: the replicated parameters are mu_cov's, handled by
        // k_cov_step; its per-target parameters are shard-local and count on every rank)
        if ((int)bid < n_target_blocks && c.not_loss_owner && !c.n_cov) loss_fin = 0.0;
        const double tot = block_sum(loss_fin, scratch);
        if (threadIdx.x == 0) {
            if (lp_early && (int)bid < n_target_blocks) {
                // this block's prior / entropy terms and its share of the guide kernel's loss parts in
                // one set of integer atomics
                long long a = lp3[0], b = lp3[1], d = lp3[2];
                if (fabs(tot) < kLossPartMax) {
                    const double hi = rint(tot * 1024.0);
                    a += (long long)hi;
                    b += (long long)rint((tot - hi * (1.0 / 1024.0)) * 1099511627776.0);
                } else {
                    d += 1;
                }
                long long* acc = c.loss_acc + ((long)ctr.slot * kLossSub + (bid & (kLossSub - 1))) * kLossWords;
                atomicAdd((unsigned long long*)acc, (unsigned long long)a);
                atomicAdd((unsigned long long*)acc + 1, (unsigned long long)b);
                if (d) atomicAdd((unsigned long long*)acc + 2, (unsigned long long)d);
            } else {
                loss_add(c, ctr.slot, tot);
            }
        }
        // other modes: the first blocks take 256 loss parts each
        if (c.lpart && !lp_early && (long)bid * blockDim.x < c.n_lpart) {
            __shared__ long long isum[3][16];
            long long ph = 0, pl = 0, pb = 0;
            for (long i = (long)bid * blockDim.x + threadIdx.x; i < c.n_lpart; i += (long)gridDim.x * blockDim.x) {
                ph += c.lpart[3 * i];
                pl += c.lpart[3 * i + 1];
                pb += c.lpart[3 * i + 2];
            }
            ph = wave_sum_i64(ph);
            pl = wave_sum_i64(pl);
            pb = wave_sum_i64(pb);
            const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
            if (lane == 0) {
                isum[0][w] = ph;
                isum[1][w] = pl;
                isum[2][w] = pb;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                long long a = 0, b = 0, d = 0;
                for (int i = 0; i < nw; ++i) {
                    a += isum[0][i];
                    b += isum[1][i];
                    d += isum[2][i];
                }
                long long* acc = c.loss_acc + ((long)ctr.slot * kLossSub + (bid & (kLossSub - 1))) * kLossWords;
                atomicAdd((unsigned long long*)acc, (unsigned long long)a);
                atomicAdd((unsigned long long*)acc + 1, (unsigned long long)b);
                if (d) atomicAdd((unsigned long long*)acc + 2, (unsigned long long)d);
            }
        }
    }
    (void)loss_prep;
    BEAN_STAMP_KP(7);
    if (PREP && FINISH) BEAN_STAMP_RT(bid, 7);
    if (bid == 0 && threadIdx.x == 0) {
        StepCtr nxt;
        nxt.step = s_prep;
        nxt.slot = slot_prep;
        nxt.step_size = 0.f;
        nxt.pad_ = 0.f;
        *c.ctrB = nxt;
    }
