// BatchNorm2d forward / backward (NHWC), single device: nn.BatchNorm2d of ir:158-159
// (eps 1e-5, momentum 0.1, affine, running statistics) + the fused ReLU / LeakyReLU(0.2) /
// residual add, and their autograd backward.
//
// Statistics are per channel over a GROUP of consecutive samples (G groups of N / G samples,
// include/irgan.h).  Same structure as norm.hip: HBM-bound row passes in which a thread owns 8
// consecutive channels (16-byte bf16 / 2 x 16-byte fp32 loads; a scalar form for C % 8 != 0 or
// unaligned slices), one partial pair per (block, channel), and a finalize launch that sums
// the partials of a group in fp64 in a fixed order -- no atomics anywhere, the gamma / beta
// gradients included.  The tables stay per (n, c) (each sample carries its group's entry), so
// the apply / backward passes and the fused resample consumers index them as InstanceNorm's;
// the statistics table holds {mean, rstd, mean_lo, 0} (the mean as a two-float sum).
//
// SyncBN (nn.SyncBatchNorm's semantics over data-parallel ranks): the same passes cut between
// "sum locally" and "finish from sums".  The local halves leave the fp64 group sums and the
// group's local element count in one buffer (sums[G][C][2], cnt[G]: include/irgan.h), the
// caller adds the buffers of all ranks, and the finishing halves run bn_group_finish / the
// backward means on the reduced values -- the arithmetic of the local kernels, so one rank's
// sums finished give the local path's bits.
#include "norm_rows.h"

namespace {

constexpr int BN_PARTS = 128;   // row-pass blocks per image: 128 double2 partials fill the work size
static_assert(2 * BN_PARTS <= IRGAN_IN_PARTS, "work buffer: IRGAN_IN_PARTS doubles per (n, c)");

// the affine output gamma * xhat + beta: ONE expression for the forward and for the backward's
// activation mask, so both see the same sign
IRGAN_HD float bn_affine(float xh, float g, float b) { return fmaf(g, xh, b); }
// xhat from the table entry {mean, rstd, mean_lo}: the mean as a two-float sum, so that its
// fp32 rounding (half an ulp of |mean|) does not reach xhat when |mean| >> the deviation
IRGAN_HD float bn_xhat(float x, float mean, float mlo, float rstd) { return ((x - mean) - mlo) * rstd; }

// Forward statistics: double2 partials {sum x, sum x^2} per (block, channel), accumulated in
// fp64 from the first add on (the products of two floats are exact in fp64), so neither a mean
// that is large against the deviation nor a long sum costs accuracy; the pass stays HBM-bound
// (three fp64 operations per loaded element).  Block layout as bn_rows_kernel.
template <int VW>
__global__ __launch_bounds__(TPB) void bn_stats_kernel(Slice X, int HW, int C, int rows_per_block,
                                                       double2* __restrict__ part) {
    __shared__ double s0[TPB * VW], s1[TPB * VW];
    const int n = blockIdx.y;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(HW, r0 + rows_per_block);
    // Lay's values (norm_rows.h: keep the two spellings equal), written out here and handed to
    // Lay: computed in Lay's constructor, or in any helper, bn_stats_kernel<8> and
    // bn_rows_kernel<1, 8> allocate a few registers more and lose a wave of occupancy each
    // (measured, profiles/norm_rows_refactor.txt; the cause was not looked for further)
    int CL = (C + VW - 1) / VW;
    if (CL > TPB) CL = TPB;
    const int RP = TPB / CL, cl = threadIdx.x % CL, rl = threadIdx.x / CL;
    const Lay L(CL, RP, cl, rl);
    for (int cb = 0; cb < C; cb += CL * VW) {
        const int c = cb + cl * VW;
        const bool on = rl < RP && c < C;   // VW == 8 only with C % 8 == 0: c + 8 <= C
        double a0[VW], a1[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) { a0[k] = 0.0; a1[k] = 0.0; }
        if (on) {
#pragma unroll 4
            for (int r = r0 + rl; r < r1; r += RP) {
                float xv[VW];
                ldw<VW>(X.p, X.dt, ((long)n * HW + r) * X.ld + X.off + c, xv);
#pragma unroll
                for (int k = 0; k < VW; ++k) {
                    const double d = (double)xv[k];
                    a0[k] += d;
                    a1[k] = fma(d, d, a1[k]);
                }
            }
        }
        // ROWS_CHAINS even where the tree would be legal: the order is the result
        block_reduce<double, VW>(a0, a1, L, ROWS_CHAINS, on, cb, c, C, s0, s1,
                                 [=](int cc, int k, double t0, double t1) {
            part[((long)n * gridDim.x + blockIdx.x) * C + cc + k] = make_double2(t0, t1);
        });
    }
}

// MODE 1: float2 partials {sum g, sum g * xhat}; MODE 2: dx (no partials), the means from the
// red table; MODE 3 (SyncBN): dx, the means formed here from the REDUCED fp64 sums -- `red` then
// points at a sync buffer (sums[G][C] double2, cnt[G]), NG = samples per group.  The two fp64
// divisions per channel are bn_bwd_finalize_kernel's expressions (one rank: its bits); they cost
// bn_rows_kernel<3, 8> 2 VGPRs over <2, 8> (140 / 138, the same waves per SIMD) and leave the
// other instantiations' allocation as it was.
// Block: CL lanes across the channels (VW each), RP rows in parallel; grid (blocks per image, N).
template <int MODE, int VW>
__global__ __launch_bounds__(TPB) void bn_rows_kernel(Slice X, Slice DY, Slice DY2, int act,
                                                      const float* __restrict__ mr, const float* __restrict__ red,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      void* dx, int dxdt, int lddx, int dxoff, int HW, int C,
                                                      int rows_per_block, float2* __restrict__ part, int NG) {
    __shared__ float s0[TPB * VW], s1[TPB * VW];
    const int n = blockIdx.y;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(HW, r0 + rows_per_block);
    int CL = (C + VW - 1) / VW;   // Lay's values, written out as in bn_stats_kernel
    if (CL > TPB) CL = TPB;
    const int RP = TPB / CL, cl = threadIdx.x % CL, rl = threadIdx.x / CL;
    const Lay L(CL, RP, cl, rl);
    for (int cb = 0; cb < C; cb += CL * VW) {
        const int c = cb + cl * VW;
        const bool on = rl < RP && c < C;   // VW == 8 only with C % 8 == 0: c + 8 <= C
        float a0[VW], a1[VW], mean[VW], mlo[VW], rstd[VW], ga[VW], be[VW], mg[VW], mgx[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) { a0[k] = 0.f; a1[k] = 0.f; }
        if (on) {
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                const float4 st = ((const float4*)mr)[(long)n * C + c + k];
                mean[k] = st.x; rstd[k] = st.y; mlo[k] = st.z; ga[k] = gamma[c + k]; be[k] = beta[c + k];
                if (MODE == 2) {
                    const float2 rd = ((const float2*)red)[(long)n * C + c + k];
                    mg[k] = rd.x; mgx[k] = rd.y;
                }
                if (MODE == 3) {
                    const int grp = n / NG, G = gridDim.y / NG;
                    const double cnt = ((const double*)red)[2L * G * C + grp];
                    const double2 e = ((const double2*)red)[(long)grp * C + c + k];
                    mg[k] = (float)(e.x / cnt); mgx[k] = (float)(e.y / cnt);
                }
            }
#pragma unroll 4
            for (int r = r0 + rl; r < r1; r += RP) {
                const long p = (long)n * HW + r;
                float xv[VW];
                ldw<VW>(X.p, X.dt, p * X.ld + X.off + c, xv);
                float gv[VW], g2[VW], o[VW];
                ldw<VW>(DY.p, DY.dt, p * DY.ld + DY.off + c, gv);
                if (DY2.p) {
                    ldw<VW>(DY2.p, DY2.dt, p * DY2.ld + DY2.off + c, g2);
#pragma unroll
                    for (int k = 0; k < VW; ++k) gv[k] += g2[k];
                }
#pragma unroll
                for (int k = 0; k < VW; ++k) {
                    const float xh = bn_xhat(xv[k], mean[k], mlo[k], rstd[k]);
                    const float g = gv[k] * act_grad(bn_affine(xh, ga[k], be[k]), act);
                    if (MODE == 1) { a0[k] += g; a1[k] += g * xh; }
                    else o[k] = ga[k] * rstd[k] * (g - mg[k] - xh * mgx[k]);
                }
                if (MODE >= 2) stw<VW>(dx, dxdt, p * lddx + dxoff + c, o);
            }
        }
        if (MODE >= 2) continue;   // uniform across the block
        // ROWS_CHAINS even where the tree would be legal: the order is the result
        block_reduce<float, VW>(a0, a1, L, ROWS_CHAINS, on, cb, c, C, s0, s1,
                                [=](int cc, int k, float t0, float t1) {
            part[((long)n * gridDim.x + blockIdx.x) * C + cc + k] = make_float2(t0, t1);
        });
    }
}

// fp64 sums {s, q} (where sub == 0) of the cnt = NG * nb partials of group grp of a channel, in
// lane_combine's order.  The groups run one after the other (the running buffers take them in
// order), so the barrier first: the previous group's reads of sm.
template <typename P2>
IRGAN_HD void group_sums(const P2* __restrict__ part, int grp, int cnt, int C, int c, int sub, int cl,
                         double (*sm)[FS][FC], double& s, double& q) {
    const P2* p = part + (long)grp * cnt * C + c;   // images grp*NG .. of nb partials each: contiguous
    double v[2];
    __syncthreads();
    lane_combine<2>(cnt, c < C, sub, cl, sm, v, [=](int j, double* t) {
        const P2 e = p[(long)j * C];
        t[0] += e.x;
        t[1] += e.y;
    });
    s = v[0];
    q = v[1];
}

// One group's statistics of a channel from its fp64 sums {s, q} over cnt elements: the table
// entry {mean, rstd, mean_lo}, the {shift b, scale a} pair (want_ab) and the unbiased variance
// the running buffers take.  ONE function for bn_finalize_kernel and bn_sync_finalize_kernel:
// the local and the synchronised path finish a group with the same operations.
struct BnGroup {
    float mean, rstd, mlo, a, b, unb;
};
IRGAN_HD BnGroup bn_group_finish(double s, double q, double cnt, float eps, bool want_ab,
                                 const float* __restrict__ gamma, const float* __restrict__ beta, int c) {
    BnGroup r;
    const double mean = s / cnt;
    double var = q / cnt - mean * mean;
    if (var < 0) var = 0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    r.mean = (float)mean;
    r.rstd = (float)rstd;
    r.mlo = (float)(mean - (double)r.mean);
    r.a = 0.f;
    r.b = 0.f;
    if (want_ab) {   // y = x * a + b, from the ROUNDED table the apply pass uses
        r.a = gamma[c] * r.rstd;
        r.b = (float)((double)beta[c] - mean * (double)r.a);
    }
    r.unb = (float)(cnt > 1.0 ? var * cnt / (cnt - 1.0) : var);
    return r;
}
// the group's entry into the tables of its samples n0 .. n0 + NG - 1
IRGAN_HD void bn_group_store(const BnGroup& r, int n0, int NG, int C, int c, float* __restrict__ mr,
                             float* __restrict__ ab) {
    for (int i = 0; i < NG; ++i) {
        const long e = (long)(n0 + i) * C + c;
        ((float4*)mr)[e] = make_float4(r.mean, r.rstd, r.mlo, 0.f);
        if (ab) ((float2*)ab)[e] = make_float2(r.b, r.a);
    }
}
// as nn.BatchNorm2d: fp32 buffers, one update per forward
IRGAN_HD void bn_running_update(float& rm, float& rv, float momentum, const BnGroup& r, int repeat) {
    for (int i = 0; i < repeat; ++i) {
        rm = (1.f - momentum) * rm + momentum * r.mean;
        rv = (1.f - momentum) * rv + momentum * r.unb;
    }
}

// forward statistics from {sum x, sum x^2} partials: P2 = double2 (bn_stats_kernel) or float2
// (irgan_conv_fwd_stats)
template <typename P2>
__global__ __launch_bounds__(FC * FS) void bn_finalize_kernel(const P2* __restrict__ part, int N, int C,
                                                              int nb, int HW, int G, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* rmean, float* rvar,
                                                              float momentum, float eps, int repeat,
                                                              float* __restrict__ mr, float* __restrict__ ab) {
    __shared__ double sm[2][FS][FC];
    const int cl = threadIdx.x % FC, sub = threadIdx.x / FC, c = blockIdx.x * FC + cl;
    const int NG = N / G;
    const bool own = sub == 0 && c < C;
    float rm = 0.f, rv = 0.f;
    if (own && rmean) { rm = rmean[c]; rv = rvar[c]; }
    for (int grp = 0; grp < G; ++grp) {
        double s, q;
        group_sums(part, grp, NG * nb, C, c, sub, cl, sm, s, q);
        if (!own) continue;
        const BnGroup r = bn_group_finish(s, q, (double)NG * HW, eps, ab != nullptr, gamma, beta, c);
        bn_group_store(r, grp * NG, NG, C, c, mr, ab);
        if (rmean) bn_running_update(rm, rv, momentum, r, repeat);
    }
    if (own && rmean) { rmean[c] = rm; rvar[c] = rv; }
}

// ---- SyncBN halves.  Buffer of a layer: sums[G][C] double2, then cnt[G] (G * (2C + 1) doubles).

// Local half of the forward (P2 = double2 / float2 as bn_finalize_kernel: {sum x, sum x^2}) and
// of the backward (float2 {sum g, sum g * xhat}; dbeta / dgamma += the LOCAL sums over all groups,
// as bn_bwd_finalize_kernel): the group sums in group_sums' order and the local element count.
template <typename P2>
__global__ __launch_bounds__(FC * FS) void bn_sync_sums_kernel(const P2* __restrict__ part, int N, int C, int nb,
                                                               int HW, int G, double* __restrict__ out,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double sm[2][FS][FC];
    const int cl = threadIdx.x % FC, sub = threadIdx.x / FC, c = blockIdx.x * FC + cl;
    const int NG = N / G;
    const bool own = sub == 0 && c < C;
    double ts = 0.0, tq = 0.0;
    for (int grp = 0; grp < G; ++grp) {
        double s, q;
        group_sums(part, grp, NG * nb, C, c, sub, cl, sm, s, q);
        if (!own) continue;
        ts += s;
        tq += q;
        ((double2*)out)[(long)grp * C + c] = make_double2(s, q);
        if (c == 0) out[2L * G * C + grp] = (double)NG * HW;
    }
    if (own) {
        if (dbeta) dbeta[c] += (float)ts;
        if (dgamma) dgamma[c] += (float)tq;
    }
}

// Finishing half of the forward: a thread per channel, the groups in order, from the REDUCED
// buffer (the count is the reduced one: no world size, uneven shards stay right).
__global__ __launch_bounds__(64) void bn_sync_finalize_kernel(const double* __restrict__ sums, int N, int C, int G,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* rmean, float* rvar,
                                                              float momentum, float eps, int repeat,
                                                              float* __restrict__ mr, float* __restrict__ ab) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const int NG = N / G;
    float rm = 0.f, rv = 0.f;
    if (rmean) { rm = rmean[c]; rv = rvar[c]; }
    for (int grp = 0; grp < G; ++grp) {
        const double2 e = ((const double2*)sums)[(long)grp * C + c];
        const BnGroup r = bn_group_finish(e.x, e.y, sums[2L * G * C + grp], eps, ab != nullptr, gamma, beta, c);
        bn_group_store(r, grp * NG, NG, C, c, mr, ab);
        if (rmean) bn_running_update(rm, rv, momentum, r, repeat);
    }
    if (rmean) { rmean[c] = rm; rvar[c] = rv; }
}

// backward means: red[n][c] = the group's {mean g, mean g * xhat} (zeros in eval mode, where the
// statistics do not depend on x); dbeta / dgamma += the sums over all groups
__global__ __launch_bounds__(FC * FS) void bn_bwd_finalize_kernel(const float2* __restrict__ part, int N, int C, int nb,
                                                                  int HW, int G, int eval, float* __restrict__ red,
                                                                  float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta) {
    __shared__ double sm[2][FS][FC];
    const int cl = threadIdx.x % FC, sub = threadIdx.x / FC, c = blockIdx.x * FC + cl;
    const int NG = N / G;
    const bool own = sub == 0 && c < C;
    double ts = 0.0, tq = 0.0;
    for (int grp = 0; grp < G; ++grp) {
        double s, q;
        group_sums(part, grp, NG * nb, C, c, sub, cl, sm, s, q);
        if (!own) continue;
        ts += s;
        tq += q;
        const double cnt = (double)NG * HW;
        const float m0 = eval ? 0.f : (float)(s / cnt), m1 = eval ? 0.f : (float)(q / cnt);
        for (int i = 0; i < NG; ++i) {
            const long e = 2 * ((long)(grp * NG + i) * C + c);
            red[e] = m0;
            red[e + 1] = m1;
        }
    }
    if (own) {
        if (dbeta) dbeta[c] += (float)ts;
        if (dgamma) dgamma[c] += (float)tq;
    }
}

__global__ __launch_bounds__(TPB) void bn_eval_table_kernel(const float* __restrict__ rmean, const float* __restrict__ rvar,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            int N, int C, float eps, float* __restrict__ mr,
                                                            float* __restrict__ ab) {
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= C) return;
    const float mean = rmean[c];
    const float rstd = (float)(1.0 / sqrt((double)rvar[c] + (double)eps));
    const float a = gamma[c] * rstd;
    const float b = (float)((double)beta[c] - (double)mean * (double)a);
    for (int n = 0; n < N; ++n) {
        const long e = (long)n * C + c;
        ((float4*)mr)[e] = make_float4(mean, rstd, 0.f, 0.f);
        if (ab) ((float2*)ab)[e] = make_float2(b, a);
    }
}

template <int VW>
__global__ __launch_bounds__(TPB) void bn_apply_kernel(Slice X, int HW, int C, const float* __restrict__ mr,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       int act, Slice R, void* __restrict__ y, int ldy, int yoff,
                                                       long total) {
    const int CV = C / VW;
    for (long idx = blockIdx.x * (long)TPB + threadIdx.x; idx < total; idx += (long)gridDim.x * TPB) {
        const long p = idx / CV;
        const int c = (int)(idx - p * CV) * VW;
        const int n = (int)(p / HW);
        float v[VW];
        ldw<VW>(X.p, X.dt, p * X.ld + X.off + c, v);
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const float4 st = ((const float4*)mr)[(long)n * C + c + k];
            v[k] = act_fwd(bn_affine(bn_xhat(v[k], st.x, st.z, st.y), gamma[c + k], beta[c + k]), act);
        }
        if (R.p) {
            float rv[VW];
            ldw<VW>(R.p, R.dt, p * R.ld + R.off + c, rv);
#pragma unroll
            for (int k = 0; k < VW; ++k) v[k] += rv[k];
        }
        stw<VW>(y, X.dt, p * ldy + yoff + c, v);
    }
}

// grid of a row pass: >= 8 rows per thread, <= BN_PARTS partials per image
RowGrid bn_grid(int N, int HW, int C, bool vec) { return row_grid(N, HW, C, vec ? V : 1, 8, BN_PARTS); }

}  // namespace

extern "C" int irgan_bn_finalize(const void* part, int32_t N, int32_t HW, int32_t C, int32_t nb, int32_t G,
                                 const float* gamma, const float* beta, float* running_mean, float* running_var,
                                 float momentum, float eps, int32_t repeat, float* mr, float* ab, irgan_stream_t s) {
    if ((long)N * HW * C <= 0) return 0;
    if (!part || !mr || nb < 1 || nb > IRGAN_IN_PARTS || G < 1 || N % G || repeat < 1 || (ab && (!gamma || !beta)) ||
        (!running_mean != !running_var))
        return IRGAN_EINVAL;
    bn_finalize_kernel<float2><<<irgan_cdiv(C, FC), FC * FS, 0, (hipStream_t)s>>>(
        (const float2*)part, N, C, nb, HW, G, gamma, beta, running_mean, running_var, momentum, eps, repeat, mr, ab);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_bn_stats(const void* x, int32_t dtype, int32_t N, int32_t HW, int32_t C, int32_t ld, int32_t off,
                              int32_t G, const float* gamma, const float* beta, float* running_mean,
                              float* running_var, float momentum, float eps, int32_t repeat, double* work, float* mr,
                              float* ab, irgan_stream_t s) {
    if ((long)N * HW * C <= 0) return 0;
    if (!x || !work || !mr || !dt_ok(dtype) || G < 1 || N % G || repeat < 1 || (ab && (!gamma || !beta)) ||
        (!running_mean != !running_var) || !slice_ok(C, ld, off))
        return IRGAN_EINVAL;
    hipStream_t st = (hipStream_t)s;
    const bool vec = vec_ok(C, {ld, off});
    const RowGrid rg = bn_grid(N, HW, C, vec);
    const int nb = rg.nb, rows = rg.rows;
    const Slice X{x, dtype, ld, off};
    const dim3 g(nb, N);   // nb <= BN_PARTS double2 partials per (n, c): 2 * 128 doubles of the work buffer's 256
    if (vec)
        bn_stats_kernel<V><<<g, TPB, 0, st>>>(X, HW, C, rows, (double2*)work);
    else
        bn_stats_kernel<1><<<g, TPB, 0, st>>>(X, HW, C, rows, (double2*)work);
    bn_finalize_kernel<double2><<<irgan_cdiv(C, FC), FC * FS, 0, st>>>(
        (const double2*)work, N, C, nb, HW, G, gamma, beta, running_mean, running_var, momentum, eps, repeat, mr, ab);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_bn_eval_table(const float* running_mean, const float* running_var, const float* gamma,
                                   const float* beta, int32_t N, int32_t C, float eps, float* mr, float* ab,
                                   irgan_stream_t s) {
    if ((long)N * C <= 0) return 0;
    if (!running_mean || !running_var || !gamma || !beta || !mr) return IRGAN_EINVAL;
    bn_eval_table_kernel<<<irgan_cdiv(C, TPB), TPB, 0, (hipStream_t)s>>>(running_mean, running_var, gamma, beta, N, C, eps,
                                                                        mr, ab);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_bn_apply(const void* x, int32_t dtype, int32_t N, int32_t HW, int32_t C, int32_t ldx, int32_t xoff,
                              const float* mr, const float* gamma, const float* beta, int32_t act, const void* res,
                              int32_t ldr, int32_t roff, void* y, int32_t ldy, int32_t yoff, irgan_stream_t s) {
    if ((long)N * HW * C <= 0) return 0;
    if (!x || !mr || !gamma || !beta || !y || !dt_ok(dtype) || !act_ok(act) || !slice_ok(C, ldx, xoff) ||
        !slice_ok(C, ldy, yoff) || (res && !slice_ok(C, ldr, roff)))
        return IRGAN_EINVAL;
    const bool vec = vec_ok(C, {ldx, xoff, ldy, yoff}) && (!res || vec_ok(C, {ldr, roff}));
    const int VW = vec ? V : 1;
    const long total = (long)N * HW * (C / VW);
    const int blocks = (int)std::min<long>((total + TPB - 1) / TPB, 16384);
    const Slice X{x, dtype, ldx, xoff}, R{res, dtype, ldr, roff};
    if (vec)
        bn_apply_kernel<V><<<blocks, TPB, 0, (hipStream_t)s>>>(X, HW, C, mr, gamma, beta, act, R, y, ldy, yoff, total);
    else
        bn_apply_kernel<1><<<blocks, TPB, 0, (hipStream_t)s>>>(X, HW, C, mr, gamma, beta, act, R, y, ldy, yoff, total);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_bn_backward(const void* dy, int32_t dy_dtype, int32_t lddy, int32_t dyoff, const void* dy2,
                                 int32_t dy2_dtype, int32_t lddy2, int32_t dy2off, const void* x, int32_t x_dtype,
                                 int32_t ldx, int32_t xoff, int32_t act, int32_t N, int32_t HW, int32_t C, int32_t G,
                                 int32_t eval, const float* mr, const float* gamma, const float* beta, double* work,
                                 float* red, void* dx, int32_t dx_dtype, int32_t lddx, int32_t dxoff, float* dgamma,
                                 float* dbeta, irgan_stream_t s) {
    if ((long)N * HW * C <= 0) return 0;
    if (!dy || !x || !mr || !gamma || !beta || !work || !red || !dx || !dt_ok(dy_dtype) || !dt_ok(x_dtype) ||
        !dt_ok(dx_dtype) || (dy2 && !dt_ok(dy2_dtype)) || G < 1 || N % G || !act_ok(act) ||
        !slice_ok(C, lddy, dyoff) || !slice_ok(C, ldx, xoff) || !slice_ok(C, lddx, dxoff) ||
        (dy2 && !slice_ok(C, lddy2, dy2off)))
        return IRGAN_EINVAL;
    hipStream_t st = (hipStream_t)s;
    const bool vec = vec_ok(C, {lddy, dyoff, ldx, xoff, lddx, dxoff}) && (!dy2 || vec_ok(C, {lddy2, dy2off}));
    const RowGrid rg = bn_grid(N, HW, C, vec);
    const int nb = rg.nb, rows = rg.rows;
    const Slice X{x, x_dtype, ldx, xoff}, DY{dy, dy_dtype, lddy, dyoff}, DY2{dy2, dy2_dtype, lddy2, dy2off};
    const dim3 g(nb, N);
    if (vec)
        bn_rows_kernel<1, V><<<g, TPB, 0, st>>>(X, DY, DY2, act, mr, nullptr, gamma, beta, nullptr, 0, 0, 0, HW, C,
                                                rows, (float2*)work, 0);
    else
        bn_rows_kernel<1, 1><<<g, TPB, 0, st>>>(X, DY, DY2, act, mr, nullptr, gamma, beta, nullptr, 0, 0, 0, HW, C,
                                                rows, (float2*)work, 0);
    bn_bwd_finalize_kernel<<<irgan_cdiv(C, FC), FC * FS, 0, st>>>((const float2*)work, N, C, nb, HW, G, eval, red, dgamma,
                                                                  dbeta);
    if (vec)
        bn_rows_kernel<2, V><<<g, TPB, 0, st>>>(X, DY, DY2, act, mr, red, gamma, beta, dx, dx_dtype, lddx, dxoff, HW, C,
                                                rows, nullptr, 0);
    else
        bn_rows_kernel<2, 1><<<g, TPB, 0, st>>>(X, DY, DY2, act, mr, red, gamma, beta, dx, dx_dtype, lddx, dxoff, HW, C,
                                                rows, nullptr, 0);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

// ---- SyncBN entry points ----

extern "C" int irgan_bn_sync_sums(const void* x, int32_t dtype, int32_t N, int32_t HW, int32_t C, int32_t ld,
                                  int32_t off, int32_t G, int32_t nb, double* work, double* sums, irgan_stream_t s) {
    if ((long)N * HW * C <= 0) return 0;
    if (!work || !sums || G < 1 || N % G || nb < 0 || nb > IRGAN_IN_PARTS) return IRGAN_EINVAL;
    hipStream_t st = (hipStream_t)s;
    if (nb > 0) {   // the conv epilogue's float2 partials
        bn_sync_sums_kernel<float2><<<irgan_cdiv(C, FC), FC * FS, 0, st>>>((const float2*)work, N, C, nb, HW, G, sums,
                                                                           nullptr, nullptr);
        IRGAN_LAUNCH_CHECK();
        return 0;
    }
    if (!x || !dt_ok(dtype) || !slice_ok(C, ld, off)) return IRGAN_EINVAL;
    const bool vec = vec_ok(C, {ld, off});
    const RowGrid rg = bn_grid(N, HW, C, vec);
    const Slice X{x, dtype, ld, off};
    const dim3 g(rg.nb, N);
    if (vec)
        bn_stats_kernel<V><<<g, TPB, 0, st>>>(X, HW, C, rg.rows, (double2*)work);
    else
        bn_stats_kernel<1><<<g, TPB, 0, st>>>(X, HW, C, rg.rows, (double2*)work);
    bn_sync_sums_kernel<double2><<<irgan_cdiv(C, FC), FC * FS, 0, st>>>((const double2*)work, N, C, rg.nb, HW, G, sums,
                                                                        nullptr, nullptr);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_bn_sync_finalize(const double* sums, int32_t N, int32_t C, int32_t G, const float* gamma,
                                      const float* beta, float* running_mean, float* running_var, float momentum,
                                      float eps, int32_t repeat, float* mr, float* ab, irgan_stream_t s) {
    if ((long)N * C <= 0) return 0;
    if (!sums || !mr || G < 1 || N % G || repeat < 1 || (ab && (!gamma || !beta)) || (!running_mean != !running_var))
        return IRGAN_EINVAL;
    bn_sync_finalize_kernel<<<irgan_cdiv(C, 64), 64, 0, (hipStream_t)s>>>(sums, N, C, G, gamma, beta, running_mean,
                                                                         running_var, momentum, eps, repeat, mr, ab);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_bn_sync_backward_sums(const void* dy, int32_t dy_dtype, int32_t lddy, int32_t dyoff,
                                           const void* dy2, int32_t dy2_dtype, int32_t lddy2, int32_t dy2off,
                                           const void* x, int32_t x_dtype, int32_t ldx, int32_t xoff, int32_t act,
                                           int32_t N, int32_t HW, int32_t C, int32_t G, const float* mr,
                                           const float* gamma, const float* beta, double* work, double* bsums,
                                           float* dgamma, float* dbeta, irgan_stream_t s) {
    if ((long)N * HW * C <= 0) return 0;
    if (!dy || !x || !mr || !gamma || !beta || !work || !bsums || !dt_ok(dy_dtype) || !dt_ok(x_dtype) ||
        (dy2 && !dt_ok(dy2_dtype)) || G < 1 || N % G || !act_ok(act) || !slice_ok(C, lddy, dyoff) ||
        !slice_ok(C, ldx, xoff) || (dy2 && !slice_ok(C, lddy2, dy2off)))
        return IRGAN_EINVAL;
    hipStream_t st = (hipStream_t)s;
    const bool vec = vec_ok(C, {lddy, dyoff, ldx, xoff}) && (!dy2 || vec_ok(C, {lddy2, dy2off}));
    const RowGrid rg = bn_grid(N, HW, C, vec);
    const Slice X{x, x_dtype, ldx, xoff}, DY{dy, dy_dtype, lddy, dyoff}, DY2{dy2, dy2_dtype, lddy2, dy2off};
    const dim3 g(rg.nb, N);
    if (vec)
        bn_rows_kernel<1, V><<<g, TPB, 0, st>>>(X, DY, DY2, act, mr, nullptr, gamma, beta, nullptr, 0, 0, 0, HW, C,
                                                rg.rows, (float2*)work, 0);
    else
        bn_rows_kernel<1, 1><<<g, TPB, 0, st>>>(X, DY, DY2, act, mr, nullptr, gamma, beta, nullptr, 0, 0, 0, HW, C,
                                                rg.rows, (float2*)work, 0);
    bn_sync_sums_kernel<float2><<<irgan_cdiv(C, FC), FC * FS, 0, st>>>((const float2*)work, N, C, rg.nb, HW, G, bsums,
                                                                       dgamma, dbeta);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_bn_sync_backward_dx(const void* dy, int32_t dy_dtype, int32_t lddy, int32_t dyoff,
                                         const void* dy2, int32_t dy2_dtype, int32_t lddy2, int32_t dy2off,
                                         const void* x, int32_t x_dtype, int32_t ldx, int32_t xoff, int32_t act,
                                         int32_t N, int32_t HW, int32_t C, int32_t G, const float* mr,
                                         const float* gamma, const float* beta, const double* bsums, void* dx,
                                         int32_t dx_dtype, int32_t lddx, int32_t dxoff, irgan_stream_t s) {
    if ((long)N * HW * C <= 0) return 0;
    if (!dy || !x || !mr || !gamma || !beta || !bsums || !dx || !dt_ok(dy_dtype) || !dt_ok(x_dtype) ||
        !dt_ok(dx_dtype) || (dy2 && !dt_ok(dy2_dtype)) || G < 1 || N % G || !act_ok(act) ||
        !slice_ok(C, lddy, dyoff) || !slice_ok(C, ldx, xoff) || !slice_ok(C, lddx, dxoff) ||
        (dy2 && !slice_ok(C, lddy2, dy2off)))
        return IRGAN_EINVAL;
    hipStream_t st = (hipStream_t)s;
    const bool vec = vec_ok(C, {lddy, dyoff, ldx, xoff, lddx, dxoff}) && (!dy2 || vec_ok(C, {lddy2, dy2off}));
    const RowGrid rg = bn_grid(N, HW, C, vec);
    const Slice X{x, x_dtype, ldx, xoff}, DY{dy, dy_dtype, lddy, dyoff}, DY2{dy2, dy2_dtype, lddy2, dy2off};
    const dim3 g(rg.nb, N);
    if (vec)
        bn_rows_kernel<3, V><<<g, TPB, 0, st>>>(X, DY, DY2, act, mr, (const float*)bsums, gamma, beta, dx, dx_dtype,
                                                lddx, dxoff, HW, C, rg.rows, nullptr, N / G);
    else
        bn_rows_kernel<3, 1><<<g, TPB, 0, st>>>(X, DY, DY2, act, mr, (const float*)bsums, gamma, beta, dx, dx_dtype,
                                                lddx, dxoff, HW, C, rg.rows, nullptr, N / G);
    IRGAN_LAUNCH_CHECK();
    return 0;
}
