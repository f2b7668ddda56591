// The body of k_sum_q (bean_kernels.hpp) and of k_sum_q_ens (bean_survival_ensemble.hpp): NOT a header of its own - it
// is included INSIDE a kernel that has `DevArgs c` in scope (text, like bean_param_body.hpp).  blockIdx.x is the replicate.
#ifndef BEAN_SUM_Q_BODY_INCLUDED_BY_KERNEL
#error "bean_sum_q_body.hpp is the text of a kernel body: include it from inside k_sum_q / k_sum_q_ens only"
#endif
    __shared__ double scratch[16];
    const int r = blockIdx.x;
    double v = 0.0;
    for (int g = threadIdx.x; g < c.G; g += blockDim.x) {
        const double gm = c.gam[(long)r * c.G + g];
        const double x = c.x0_in ? gm
                                 : (double)fminf(fmaxf((float)(gm * frcp(c.gsum[r])), 1.17549435e-38f), 0.99999994f);
        v += x * c.gq[(long)r * c.G + g];
    }
    const double tot = block_sum(v, scratch);
    if (threadIdx.x == 0) c.sq[r] = tot;
