// InstanceNorm forward / backward and channel reductions (NHWC, per (n, c)
// over H*W).  Replaces nn.InstanceNorm2d (ir:154-165: eps 1e-5, no affine, no
// running stats) + the fused ReLU / LeakyReLU(0.2) / residual add of ir:392,
// 417-418, 601-624 and their autograd backward.
//
// HBM-bound: every thread owns 8 consecutive channels (one 16-byte bf16 load /
// two 16-byte fp32 loads per pixel) and walks >= 8 rows; a block covers a run of
// rows of one image and reduces its partial sums through LDS.  Reductions are
// two-level and atomic-free: each block stores one float2 partial per channel
// (<= IN_PARTS blocks per image), and the finalize launch sums the partials of
// each (n, c) in fp64, in a fixed order (deterministic), into fp32 (mean, rstd)
// or (mean g, mean g*xhat).  The pieces of a row pass -- the layout, the loads, the grid and
// the order of every reduction -- are norm_rows.h's, shared with batchnorm.hip.
#include "fp8_util.h"
#include "norm_rows.h"

namespace {

// optional fp8 copy of a pass's bf16 output (the fp8 path's conv operands,
// GeneratorEngine(fp8=True)): y8 = e4m3(clamp(bf16(y) * q[0])), max |bf16(y)|
// into the amax slot -- the same bytes irgan_fp8_quant makes from the stored y
struct Q8 {
    uint8_t* p;
    int ld, off;
    const float* q;
    uint32_t* amax;
};

constexpr int IN_PARTS = 128; // max rows-kernel blocks (partials) per image (<= IRGAN_IN_PARTS, the work size)

// MODE 0: (sum x, sum x^2); MODE 1: (sum g, sum g*xhat), g = (dy+dy2)*act'(xhat),
// xhat = (x-mean)*rstd;  MODE 2: MODE-1 pass that also writes dx and sums dx (db)
template <int MODE, int VW>
__global__ __launch_bounds__(TPB) void rows_kernel(Slice X, Slice DY, Slice DY2, int act, const float* __restrict__ mr,
                                                   const float* __restrict__ red, void* __restrict__ dx, int dxdt,
                                                   int lddx, int dxoff, int HW, int C, int rows_per_block,
                                                   float2* __restrict__ part, float* __restrict__ db) {
    __shared__ float s0[TPB * VW], s1[TPB * VW];
    const int n = blockIdx.y;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(HW, r0 + rows_per_block);
    Lay L(C, VW);
    const bool active = L.rl < L.RP;
    for (int cb = 0; cb < C; cb += L.CL * VW) {
        const int c = cb + L.cl * VW;
        const bool on = active && c < C;
        float a0[VW], a1[VW], mean[VW], rstd[VW], mg[VW], mgx[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) { a0[k] = 0.f; a1[k] = 0.f; }
        if (on && MODE >= 1) {
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                const float2 st = ((const float2*)mr)[(long)n * C + c + k];
                mean[k] = st.x; rstd[k] = st.y;
                if (MODE == 2) {
                    const float2 rd = ((const float2*)red)[(long)n * C + c + k];
                    mg[k] = rd.x; mgx[k] = rd.y;
                }
            }
        }
        if (on) {
#pragma unroll 8
            for (int r = r0 + L.rl; r < r1; r += L.RP) {
                const long p = (long)n * HW + r;
                float xv[VW];
                ldw<VW>(X.p, X.dt, p * X.ld + X.off + c, xv);
                if (MODE == 0) {
#pragma unroll
                    for (int k = 0; k < VW; ++k) { a0[k] += xv[k]; a1[k] += xv[k] * xv[k]; }
                } else {
                    float gv[VW], g2[VW];
                    ldw<VW>(DY.p, DY.dt, p * DY.ld + DY.off + c, gv);
                    if (DY2.p) {
                        ldw<VW>(DY2.p, DY2.dt, p * DY2.ld + DY2.off + c, g2);
#pragma unroll
                        for (int k = 0; k < VW; ++k) gv[k] += g2[k];
                    }
                    float o[VW];
#pragma unroll
                    for (int k = 0; k < VW; ++k) {
                        const float xh = (xv[k] - mean[k]) * rstd[k];
                        const float g = gv[k] * act_grad(xh, act);
                        if (MODE == 1) { a0[k] += g; a1[k] += g * xh; }
                        else { o[k] = rstd[k] * (g - mg[k] - xh * mgx[k]); a0[k] += o[k]; }
                    }
                    if (MODE == 2) stw<VW>(dx, dxdt, p * lddx + dxoff + c, o);
                }
            }
        }
        if (MODE == 2 && !db) continue;  // uniform across the block
        block_reduce<float, VW>(a0, a1, L, in_row_order(L.CL), on, cb, c, C, s0, s1,
                                [=](int cc, int k, float t0, float t1) {
            if (MODE == 2) atomicAdd(db + cc + k, t0);
            else part[((long)n * gridDim.x + blockIdx.x) * C + cc + k] = make_float2(t0, t1);   // block b of image n
        });
    }
}

// All-bf16 fast path of rows_kernel<MODE, 8> for MODE 0 (stats), 1 (backward
// reduce) and 2 (backward apply without db), and MODE 4: the forward apply
// y = act((x - mean) * rstd) [+ res] (res in the dy slot, nullable) -- apply_kernel's job
// without its per-element index divisions and per-element {mean, rstd} reloads: a
// thread's 8 channels and image are fixed, so their table entries are loaded once.  rows_kernel issues one row's
// loads at a time at ~150 VGPRs (3 waves per SIMD), so only ~24 KB of loads are
// in flight per CU and the backward reduce streams at ~2 TB/s.  Here each
// thread walks its rows in batches of U and issues every 16-byte load of a
// batch, unconverted, before using any; tail rows of the last batch re-load a
// valid row and are masked.  dx may alias dy (no __restrict__ on either): a
// thread stores only rows it has already loaded.  The loads stay raw uint4 (not ldw, whose
// conversion would sit between them).
// One batch at a time: two register batches in flight (U rows each, the next batch's loads
// issued before the current one is used) measured no faster standalone (tools/norm_bench.py)
// and -0.5 % on the step on the same box (profiles/r05_s5_nab.txt).
// The eval-mode forms of the fp8 forward apply (F8, MODE 4; irgan_in_apply_fp8): AMAX false
// records nothing -- no running maximum, no fp8_block_amax, so no atomic and no trailing
// barrier; Y16 false (with AMAX false only) writes the e4m3 copy alone, without the 16-byte bf16
// store (the value is still rounded to bf16 first, so the bytes are those of the full call).
template <int MODE, int U, bool F8 = false, bool AMAX = true, bool Y16 = true>
__global__ __launch_bounds__(TPB) void rows8_kernel(const bf16_t* x, int ldx, int xoff, const bf16_t* dy, int lddy,
                                                    int dyoff, const bf16_t* dy2, int lddy2, int dy2off, int act,
                                                    const float* __restrict__ mr, const float* __restrict__ red,
                                                    bf16_t* dx, int lddx, int dxoff, int HW, int C, int rows_per_block,
                                                    float2* __restrict__ part, Q8 q8) {
    __shared__ float s0[TPB * 8], s1[TPB * 8];
    const float qs = F8 ? *q8.q : 1.f;
    float amx = 0.f;
    const int n = blockIdx.y;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(HW, r0 + rows_per_block);
    Lay L(C, 8);
    const bool active = L.rl < L.RP;
    const long pb = (long)n * HW;
    for (int cb = 0; cb < C; cb += L.CL * 8) {
        const int c = cb + L.cl * 8;
        const bool on = active && c < C;
        float a0[8], a1[8], mean[8], rstd[8], mg[8], mgx[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { a0[k] = 0.f; a1[k] = 0.f; }
        if (on && MODE >= 1) {   // (MODE 4 as well)
            const float4* m4 = (const float4*)(mr + 2 * ((long)n * C + c));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 t = m4[k];
                mean[2 * k] = t.x; rstd[2 * k] = t.y; mean[2 * k + 1] = t.z; rstd[2 * k + 1] = t.w;
            }
            if (MODE == 2) {
                const float4* r4 = (const float4*)(red + 2 * ((long)n * C + c));
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 t = r4[k];
                    mg[2 * k] = t.x; mgx[2 * k] = t.y; mg[2 * k + 1] = t.z; mgx[2 * k + 1] = t.w;
                }
            }
        }
        if (on) {
            uint4 xr[U], gr[U], hr[U];
            auto load = [&](int r) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const long p = pb + min(r + u * L.RP, r1 - 1);
                    xr[u] = *(const uint4*)(x + p * ldx + xoff + c);
                    if (MODE != 0 && (MODE != 4 || dy)) gr[u] = *(const uint4*)(dy + p * lddy + dyoff + c);
                }
                if (MODE != 0 && dy2) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const long p = pb + min(r + u * L.RP, r1 - 1);
                        hr[u] = *(const uint4*)(dy2 + p * lddy2 + dy2off + c);
                    }
                }
            };
            auto process = [&](int r) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (r + u * L.RP >= r1) break;
                    float xv[8];
                    bf8f(xr[u], xv);
                    if (MODE == 0) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) { a0[k] += xv[k]; a1[k] += xv[k] * xv[k]; }
                        continue;
                    }
                    float gv[8];
                    if (MODE != 4 || dy) bf8f(gr[u], gv);
                    if (dy2) {
                        float hv[8];
                        bf8f(hr[u], hv);
#pragma unroll
                        for (int k = 0; k < 8; ++k) gv[k] += hv[k];
                    }
                    float o[8];
                    if (MODE == 4) {   // forward apply (as apply_kernel, same float ops)
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const float h = act_fwd((xv[k] - mean[k]) * rstd[k], act);
                            o[k] = dy ? h + gv[k] : h;
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const float xh = (xv[k] - mean[k]) * rstd[k];
                            const float g = gv[k] * act_grad(xh, act);
                            if (MODE == 1) { a0[k] += g; a1[k] += g * xh; }
                            else o[k] = rstd[k] * (g - mg[k] - xh * mgx[k]);
                        }
                    }
                    if (MODE == 2 || MODE == 4) {
                        uint4 w;
                        w.x = pk_bf16(o[0], o[1]);
                        w.y = pk_bf16(o[2], o[3]);
                        w.z = pk_bf16(o[4], o[5]);
                        w.w = pk_bf16(o[6], o[7]);
                        if constexpr (Y16) *(uint4*)(dx + (pb + r + u * L.RP) * lddx + dxoff + c) = w;
                        if constexpr (F8) {
                            float vb[8];
                            bf8f(w, vb);
                            if constexpr (AMAX) {
#pragma unroll
                                for (int k = 0; k < 8; ++k) amx = fmaxf(amx, fabsf(vb[k]));
                            }
                            *(uint2*)(q8.p + (pb + r + u * L.RP) * q8.ld + q8.off + c) = pack8_fp8(vb, qs);
                        }
                    }
                }
            };
            const int step = U * L.RP;
#pragma unroll 1
            for (int r = r0 + L.rl; r < r1; r += step) {
                load(r);
                process(r);
            }
        }
        if (MODE == 2 || MODE == 4) continue;  // uniform across the block
        block_reduce<float, 8>(a0, a1, L, in_row_order(L.CL), on, cb, c, C, s0, s1,
                               [=](int cc, int k, float t0, float t1) {
            part[((long)n * gridDim.x + blockIdx.x) * C + cc + k] = make_float2(t0, t1);
        });
    }
    if constexpr (F8 && AMAX) fp8_block_amax(amx, q8.amax, blockIdx.y * gridDim.x + blockIdx.x);
}

// Rows per thread and rows per load batch (U) of each pass, by key: 0 stats, 1 backward
// reduce, 2 backward apply, 4 forward apply, 5 forward apply + residual / with the fp8 copy.
// Measured at the resblock shape, B = 16 (profiles/r05_nsw_norm_sweep.txt, swept through
// per-pass overrides that have since gone): forward apply 16.2 -> 14.4 us and backward
// apply 17.9 -> 17.5 at 4 rows per thread in one batch; the reduce stays at 16 rows in batches
// of 4 (one batch of 4: 20.7 us, 4x the partials), apply + residual at 8 rows in batches of 4
constexpr int PASS_RPT[6] = {16, 16, 4, 0, 4, 8}, PASS_U[6] = {16, 4, 4, 0, 4, 4};  // U: the batch cap (larger maps: several batches)

// What a row pass or the one-pass backward reads and writes, as the entry points fill it;
// members a pass does not use stay zero.  DY is the residual of the forward apply; q8.p == null:
// no fp8 copy.
struct RowArgs {
    Slice X, DY, DY2;
    int act;
    const float *mr, *red;   // red: the row passes read it
    float* red_out;          // the one-pass backward writes it
    OSlice DX;
    int N, HW, C;
    float2* part;
    float* db;
    Q8 q8;
};

// The kernels keep the parent's loose parameter lists: taking the slices as structs left every
// register count alone but moved their scalar registers, and two passes then timed beyond the
// run-to-run spread (profiles/norm_rows_refactor.txt).  These two are the only places that unpack.
inline const bf16_t* bfp(const Slice& s) { return (const bf16_t*)s.p; }

// rows8_kernel with U = min(the thread's rows, the pass's batch), from the instances 2 / 4 / 8 / 16
template <int MODE, bool F8, int U, bool AMAX = true, bool Y16 = true>
void rows8_launch(const RowGrid& g, hipStream_t st, const RowArgs& a) {
    rows8_kernel<MODE, U, F8, AMAX, Y16><<<dim3(g.nb, a.N), TPB, 0, st>>>(
        bfp(a.X), a.X.ld, a.X.off, bfp(a.DY), a.DY.ld, a.DY.off, bfp(a.DY2), a.DY2.ld, a.DY2.off, a.act, a.mr, a.red,
        (bf16_t*)a.DX.p, a.DX.ld, a.DX.off, a.HW, a.C, g.rows, a.part, a.q8);
}
template <int MODE, bool F8, bool AMAX = true, bool Y16 = true>
void rows8_go(int key, const RowGrid& g, hipStream_t st, const RowArgs& a) {
    const int u = std::min(PASS_U[key], irgan_cdiv(g.rows, g.RP));
    if (u <= 2) rows8_launch<MODE, F8, 2, AMAX, Y16>(g, st, a);
    else if (u <= 4) rows8_launch<MODE, F8, 4, AMAX, Y16>(g, st, a);
    else if (u <= 8) rows8_launch<MODE, F8, 8, AMAX, Y16>(g, st, a);
    else rows8_launch<MODE, F8, 16, AMAX, Y16>(g, st, a);
}

// rows8_kernel<1> whose gradient is not loaded but made per pixel from a four times smaller one:
// da = bf16((Wy (x) Wx) dy) at pixel (oy, ox) from at most 2 x 2 taps of dy (the Downsample
// adjoint; irgan_sep_resample_in_bwd_reduce), in sep_pipe_kernel's order -- the vertical taps of
// each tap column first, then the horizontal ones, zero-weight slots skipped, fused multiply-adds
// from +0 -- so da is the bytes irgan_sep_resample stores and, the chains, block_reduce and the
// partial layout being rows8_kernel<1>'s at the same (N, HW, C), the partials are the bits the
// reduce pass over the stored da leaves.  The up-sampled gradient is never written or read; the
// taps of neighbouring pixels share their 16-byte loads in the caches.  The block's slice of the
// two tap tables (all Wout columns, the NR output rows its pixels lie in) sits in LDS, so a
// pixel's tap addresses cost no memory round trip in front of its loads.
template <int U>
__global__ __launch_bounds__(TPB) void rows8_adjoint_reduce_kernel(
    const bf16_t* __restrict__ x, int ldx, int xoff, const bf16_t* __restrict__ dy, int lddy, int dyoff, int Hin, int Win,
    int W, const int* __restrict__ ty, const float* __restrict__ wy, int Ty, const int* __restrict__ tx,
    const float* __restrict__ wx, int Tx, int act, const float* __restrict__ mr, int HW, int C, int rows_per_block,
    int NR, float2* __restrict__ part) {
    __shared__ float s0[TPB * 8], s1[TPB * 8];
    extern __shared__ float4 tab4[];
    float* const lwx = (float*)tab4;          // [W][2] horizontal weights, then taps
    int* const lix = (int*)(lwx + 2 * W);
    float* const lwy = (float*)(lix + 2 * W);   // [NR][2] vertical weights, then taps, from row oyb
    int* const liy = (int*)(lwy + 2 * NR);
    const int n = blockIdx.y;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(HW, r0 + rows_per_block);
    const int oyb = r0 / W, H = HW / W;
    for (int e = threadIdx.x; e < 2 * W; e += TPB) {
        const int o = e >> 1, i = e & 1;
        lwx[e] = i < Tx ? wx[o * Tx + i] : 0.f;
        lix[e] = i < Tx ? tx[o * Tx + i] : 0;
    }
    for (int e = threadIdx.x; e < 2 * NR; e += TPB) {
        const int o = min(oyb + (e >> 1), H - 1), i = e & 1;
        lwy[e] = i < Ty ? wy[o * Ty + i] : 0.f;
        liy[e] = i < Ty ? ty[o * Ty + i] : 0;
    }
    __syncthreads();
    Lay L(C, 8);
    const bool active = L.rl < L.RP;
    const long pb = (long)n * HW;
    const float neg = act == IRGAN_ACT_RELU ? 0.f : act == IRGAN_ACT_LRELU ? 0.2f : 1.f;   // act_grad where xhat <= 0
    for (int cb = 0; cb < C; cb += L.CL * 8) {
        const int c = cb + L.cl * 8;
        const bool on = active && c < C;
        float a0[8], a1[8], mean[8], rstd[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { a0[k] = 0.f; a1[k] = 0.f; }
        if (on) {
            const float4* m4 = (const float4*)(mr + 2 * ((long)n * C + c));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 t = m4[k];
                mean[2 * k] = t.x; rstd[2 * k] = t.y; mean[2 * k + 1] = t.z; rstd[2 * k + 1] = t.w;
            }
            uint4 xr[U], gr[U][2][2];
            float wv[U][2], wh[U][2];
            const int step = U * L.RP;
#pragma unroll 1
            for (int r = r0 + L.rl; r < r1; r += step) {
#pragma unroll
                for (int u = 0; u < U; ++u) {   // every load of the batch before any use
                    const int q = min(r + u * L.RP, r1 - 1);
                    const int oy = q / W, ox = q - oy * W;
                    xr[u] = *(const uint4*)(x + (pb + q) * ldx + xoff + c);
                    int iy[2], ix[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        wv[u][i] = lwy[2 * (oy - oyb) + i];
                        iy[i] = liy[2 * (oy - oyb) + i];
                        wh[u][i] = lwx[2 * ox + i];
                        ix[i] = lix[2 * ox + i];
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            gr[u][i][j] = wv[u][i] != 0.f && wh[u][j] != 0.f   // (a pixel has 1, 2 or 4 taps)
                                              ? *(const uint4*)(dy + (((long)n * Hin + iy[i]) * Win + ix[j]) * lddy + dyoff + c)
                                              : make_uint4(0u, 0u, 0u, 0u);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (r + u * L.RP >= r1) break;
                    float xv[8], t[2][2][8];
                    bf8f(xr[u], xv);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) bf8f(gr[u][i][j], t[i][j]);
                    float o[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        float col[2];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            col[j] = 0.f;
#pragma unroll
                            for (int i = 0; i < 2; ++i)
                                if (wv[u][i] != 0.f) col[j] = __builtin_fmaf(wv[u][i], t[i][j][k], col[j]);
                        }
                        o[k] = 0.f;
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            if (wh[u][j] != 0.f) o[k] = __builtin_fmaf(wh[u][j], col[j], o[k]);
                    }
                    uint4 w;   // the stored bf16 of the plain launch
                    w.x = pk_bf16(o[0], o[1]);
                    w.y = pk_bf16(o[2], o[3]);
                    w.z = pk_bf16(o[4], o[5]);
                    w.w = pk_bf16(o[6], o[7]);
                    float gv[8];
                    bf8f(w, gv);
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        // the contractions rows8_kernel<1> compiles to, spelled out (in_bwd_onepass_kernel)
                        const float xh = (xv[k] - mean[k]) * rstd[k];
                        const float f = xh > 0.f ? 1.f : neg;
                        a0[k] = __builtin_fmaf(gv[k], f, a0[k]);
                        a1[k] = __builtin_fmaf(gv[k] * f, xh, a1[k]);
                    }
                }
            }
        }
        block_reduce<float, 8>(a0, a1, L, in_row_order(L.CL), on, cb, c, C, s0, s1,
                               [=](int cc, int k, float t0, float t1) {
            part[((long)n * gridDim.x + blockIdx.x) * C + cc + k] = make_float2(t0, t1);
        });
    }
}

// fp64 sum of the nb block partials of each (n, c): one block (FC channels x FS partial
// lanes) per (image, channel group), the order is lane_combine's (deterministic).
__global__ __launch_bounds__(256) void finalize_kernel(const float2* __restrict__ part, float* __restrict__ mr, int N,
                                                       int C, int nb, int HW, int mode) {
    __shared__ double sm[2][FS][FC];
    const int n = blockIdx.y, cl = threadIdx.x % FC, sub = threadIdx.x / FC;
    const int c = blockIdx.x * FC + cl;
    double v[2];
    lane_combine<2>(nb, c < C, sub, cl, sm, v, [&](int b, double* t) {
        const float2 p = part[((long)n * nb + b) * C + c];
        t[0] += p.x;
        t[1] += p.y;
    });
    if (sub != 0 || c >= C) return;
    const double s = v[0], q = v[1];
    const long i = (long)n * C + c;
    const double mean = s / HW;
    if (mode == 0) {
        double var = q / HW - mean * mean;
        if (var < 0) var = 0;
        mr[2 * i] = (float)mean;
        mr[2 * i + 1] = (float)(1.0 / sqrt(var + 1e-5));
    } else {
        mr[2 * i] = (float)mean;
        mr[2 * i + 1] = (float)(q / HW);
    }
}

// forward apply for what rows8_kernel<4> does not take: fp32, scalar channels, an xhat copy
template <int VW>
__global__ __launch_bounds__(TPB) void apply_kernel(Slice X, int HW, int C, const float* __restrict__ mr, int act,
                                                    Slice R, void* __restrict__ y, int ldy, int yoff,
                                                    void* __restrict__ xhat, long total) {
    const int CV = C / VW;
    for (long idx = blockIdx.x * (long)TPB + threadIdx.x; idx < total; idx += (long)gridDim.x * TPB) {
        const long p = idx / CV;
        const int c = (int)(idx - p * CV) * VW;
        const int n = (int)(p / HW);
        float v[VW];
        ldw<VW>(X.p, X.dt, p * X.ld + X.off + c, v);
        const float4* m4 = (const float4*)(mr + 2 * ((long)n * C + c));
#pragma unroll
        for (int k = 0; k < VW; k += 2) {
            float4 st;
            if constexpr (VW == 8) st = m4[k / 2];
            else { st = make_float4(mr[2 * ((long)n * C + c)], mr[2 * ((long)n * C + c) + 1], 0.f, 0.f); }
            v[k] = (v[k] - st.x) * st.y;
            if (VW > 1) v[k + 1] = (v[k + 1] - st.z) * st.w;
        }
        if (xhat) stw<VW>(xhat, X.dt, p * C + c, v);
#pragma unroll
        for (int k = 0; k < VW; ++k) v[k] = act_fwd(v[k], act);
        if (R.p) {
            float rv[VW];
            ldw<VW>(R.p, R.dt, p * R.ld + R.off + c, rv);
#pragma unroll
            for (int k = 0; k < VW; ++k) v[k] += rv[k];
        }
        stw<VW>(y, X.dt, p * ldy + yoff + c, v);
    }
}

// The grid of pass `key` (PASS_RPT): row_grid with <= IN_PARTS partials per image.  rpt 16 for
// the reductions (stats, backward reduce: half the partials for the finalize), less for the
// passes that write -- measured per pass at the resblock shape (r03_e: backward reduce +
// finalize 20.6 -> 17.2 us, apply + ReLU 17.4 -> 16.5, apply + residual 18.1 -> 18.8, backward
// apply 18.4 -> 18.6; U = 2 / a 128-VGPR cap on the reduce: no gain)
RowGrid pass_grid(int key, int N, int HW, int C, int VW) { return row_grid(N, HW, C, VW, PASS_RPT[key], IN_PARTS); }

// Row pass MODE (0 stats, 1 backward reduce, 2 backward apply) over a's slices: rows8_kernel
// where everything is bf16 in 8-channel vectors and no db is asked for, else rows_kernel.
// Returns the number of partials per image.
template <int MODE>
int launch_rows(const RowArgs& a, bool vec, hipStream_t st) {
    const RowGrid g = pass_grid(MODE, a.N, a.HW, a.C, vec ? V : 1);
    const bool bf = a.X.dt == IRGAN_BF16 &&
                    (MODE == 0 || (a.DY.dt == IRGAN_BF16 && (!a.DY2.p || a.DY2.dt == IRGAN_BF16))) &&
                    (MODE != 2 || (a.DX.dt == IRGAN_BF16 && !a.db));
    if (vec && bf) {
        if constexpr (MODE == 2) {   // the one row pass with an fp8 instance (irgan_in_bwd_apply_fp8)
            if (a.q8.p) {
                rows8_go<2, true>(2, g, st, a);
                return g.nb;
            }
        }
        rows8_go<MODE, false>(MODE, g, st, a);
        return g.nb;
    }
    const dim3 grid(g.nb, a.N);
    if (vec)
        rows_kernel<MODE, V><<<grid, TPB, 0, st>>>(a.X, a.DY, a.DY2, a.act, a.mr, a.red, a.DX.p, a.DX.dt, a.DX.ld,
                                                   a.DX.off, a.HW, a.C, g.rows, a.part, a.db);
    else
        rows_kernel<MODE, 1><<<grid, TPB, 0, st>>>(a.X, a.DY, a.DY2, a.act, a.mr, a.red, a.DX.p, a.DX.dt, a.DX.ld,
                                                   a.DX.off, a.HW, a.C, g.rows, a.part, a.db);
    return g.nb;
}

// One-pass InstanceNorm backward for maps that fit one CU's registers.  InstanceNorm is
// independent per (image, channel), so a workgroup owns (image n, CG consecutive channels)
// instead of a run of rows: it loads its slices of x and dy once (every 16-byte load of the
// slice issued before any is used), reduces sum g and sum g*xhat itself, and writes dx from
// the registers it holds -- 6 bytes per element where reduce + finalize + apply move 10, and
// no partials, finalize launch, ticket or wait on another block.
// The result is the three launches' bit for bit: the sums are grouped exactly as
// rows8_kernel<1> + finalize_kernel group them at the same (N, HW, C), that is, as
// norm_rows.h's row_grid, block_reduce and lane_combine do.  There, block b of nb covers
// `rows` rows (row_grid, called through pass_grid by both), its thread (rl, channel lane) adds
// rows r0 + rl, r0 + rl + RP, ... in order (a chain), block_reduce combines the RP chains of a
// channel (ROWS_TREE: a butterfly inside each wave then the four waves in order, or
// ROWS_CHAINS: the RP chains in order, when the channel lanes do not divide a wave), and
// lane_combine adds the nb partials in fp64 (partial b in lane b % FS, the lanes in order).
// This kernel cannot call the two: its chains are not laid out as a row pass's block, so it
// re-enacts both orders in LDS.  Here a thread owns one chain of one channel octet (CG / 8
// octets): it holds the chain's <= U pixels, sums them in the same order with the same float
// operations (the fused multiply-adds rows8_kernel compiles to are written out), the chains
// meet in LDS and are combined in that order, and the fp32 {mean g, mean g*xhat} stored to red
// are the values dx is computed from.  Tail items re-load a valid
// pixel with dy = 0 (they add +-0).  Deterministic; no atomics but the amax record.  The
// barriers of the reduction sit between a workgroup's last load and its first store and it
// stores only pixels it loaded, so dx may alias dy.
// Logical group t = n * (C / CG) + cg runs on XCD blockIdx.x % 8 in contiguous ranges
// (xcd_tile_any): the 64 / CG groups that share the 128-byte lines of one image sit in
// adjacent dispatch slots of one L2.  Speed only, but all of it: in plain blockIdx order the
// four groups of a line sit on four XCDs and the launch takes twice as long.
// At most 512 threads (a full map: 256 chains of 16 pixels per octet, 214 VGPRs, no scratch).
// IN_ONEPASS_CG: variant builds (tools/build_variant.sh) for tools/norm_bench.py; CG = 8 reads
// 16-byte segments and is slower, CG = 32 holds 2048 px (profiles/in_bwd_onepass_bench.txt)
#ifndef IN_ONEPASS_CG
#define IN_ONEPASS_CG IRGAN_IN_ONEPASS_CG
#endif
constexpr int OP_CG = IN_ONEPASS_CG;   // channels per workgroup: 8, 16 or 32
constexpr int OP_MAXU = 16;            // pixels per chain: 16 x (x, dy) uint4 = 128 raw VGPRs per thread
constexpr int OP_MAXNT = 512;
constexpr int OP_CAP = IRGAN_IN_ONEPASS_ELEMS;   // elements of one (n, channel group) slice: 4096 px at CG = 16

template <bool F8, int NT, int CG, int U>
__global__ __launch_bounds__(NT) void in_bwd_onepass_kernel(const bf16_t* x, int ldx, int xoff, const bf16_t* dy,
                                                            int lddy, int dyoff, int act,
                                                            const float* __restrict__ mr, float* __restrict__ red,
                                                            bf16_t* dx, int lddx, int dxoff, int HW, int C, int swz,
                                                            int nb, int rows, int RP, Q8 q8) {
    constexpr int LPP = CG / 8, NCH = NT / LPP;
    static_assert(LPP == 1 || LPP == 2 || LPP == 4, "CG in {8, 16, 32}");
    __shared__ float sc[NCH][CG * 2];        // chain sums: [chain][(channel, g | g*xhat)]
    __shared__ float pt[IN_PARTS][CG * 2];   // the nb block partials of rows8_kernel<1>
    __shared__ float sf[CG][2];              // {mean g, mean g*xhat}: the values stored to red
    const int G = C / CG;
    const int t = swz ? xcd_tile_any(blockIdx.x, gridDim.x) : blockIdx.x;
    const int n = t / G, cg = t - n * G;
    const int h = threadIdx.x % LPP, q = threadIdx.x / LPP;   // channel octet, chain
    const int b = q / RP, rl = q - b * RP;
    const bool on = q < nb * RP;
    const int r0 = b * rows + rl, r1 = on ? min(HW, (b + 1) * rows) : 0;   // the chain: r0, r0 + RP, ... < r1
    // workgroup-uniform 64-bit bases (scalar registers) + 32-bit lane offsets inside the
    // image (HW * ld < 2^30, checked by the launcher)
    const long pb = (long)n * HW;
    const bf16_t* xb = x + pb * ldx + xoff + cg * CG;
    const bf16_t* gb = dy + pb * lddy + dyoff + cg * CG;
    bf16_t* ob = dx + pb * lddx + dxoff + cg * CG;
    const uint32_t h8 = h * 8;

    uint4 xr[U], gr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t p = min(r0 + u * RP, HW - 1);
        xr[u] = *(const uint4*)(xb + (p * (uint32_t)ldx + h8));
        gr[u] = *(const uint4*)(gb + (p * (uint32_t)lddy + h8));
    }
    // {mean, rstd} of the group's CG channels while those loads are in flight: the address is
    // workgroup-uniform (constant address space: the kernel never writes the table), a lane
    // selects its octet's entries
    typedef const float __attribute__((address_space(4))) * cfloat_p;
    const cfloat_p mrow = (cfloat_p)(uintptr_t)(mr + 2 * ((long)n * C + cg * CG));
    float mean[8], rstd[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        mean[k] = mrow[2 * k];
        rstd[k] = mrow[2 * k + 1];
#pragma unroll
        for (int j = 1; j < LPP; ++j) {
            mean[k] = h == j ? mrow[2 * (j * 8 + k)] : mean[k];
            rstd[k] = h == j ? mrow[2 * (j * 8 + k) + 1] : rstd[k];
        }
    }
    // act_grad(xh, act) without its per-element branches on act: 1 where xh > 0, else `neg`
    const float neg = act == IRGAN_ACT_RELU ? 0.f : act == IRGAN_ACT_LRELU ? 0.2f : 1.f;
    float a0[8], a1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { a0[k] = 0.f; a1[k] = 0.f; }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        // an item past the chain's end holds a valid pixel of the same channels: its dy becomes
        // 0, so it adds +-0 to both sums (straight-line code; rows8_kernel breaks out instead)
        if (r0 + u * RP >= r1) gr[u] = make_uint4(0u, 0u, 0u, 0u);
        float xv[8], gv[8];
        bf8f(xr[u], xv);
        bf8f(gr[u], gv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            // the contractions rows8_kernel<1> compiles to, spelled out (left to the compiler
            // here, the two sums pair into a packed add and g * xh is rounded before it)
            const float xh = (xv[k] - mean[k]) * rstd[k];
            const float f = xh > 0.f ? 1.f : neg;
            a0[k] = __builtin_fmaf(gv[k], f, a0[k]);
            a1[k] = __builtin_fmaf(gv[k] * f, xh, a1[k]);
        }
        __builtin_amdgcn_sched_barrier(0);   // one item's temporaries at a time (register budget)
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        sc[q][(h * 8 + k) * 2] = a0[k];
        sc[q][(h * 8 + k) * 2 + 1] = a1[k];
    }
    __syncthreads();
    // block_reduce of block pbk for one (channel, sum), in the order rows8_kernel asks of it
    // (in_row_order at its CL channel lanes)
    const int CL = min(C / 8, TPB);
    const bool tree = in_row_order(CL) == ROWS_TREE;
    for (int task = threadIdx.x; task < nb * CG * 2; task += NT) {
        const int cw = task % (CG * 2), pbk = task / (CG * 2);
        const int c0 = pbk * RP;
        float tsum = 0.f;
        if (tree) {
            const int RW = RP / (TPB / 64);   // rows of one wave: the butterfly, then the waves in order
            for (int j = 0; j < TPB / 64; ++j) {
                for (int o = 1; o < RW; o <<= 1)
                    for (int i = 0; i < RW; i += 2 * o) sc[c0 + j * RW + i][cw] += sc[c0 + j * RW + i + o][cw];
                tsum += sc[c0 + j * RW][cw];
            }
        } else {
            for (int j = 0; j < RP; ++j) tsum += sc[c0 + j][cw];
        }
        pt[pbk][cw] = tsum;
    }
    __syncthreads();
    if (threadIdx.x < CG * 2) {   // lane_combine: partial pbk in lane pbk % FS, then the lanes in order
        const int cw = threadIdx.x;
        double s = 0.0;
        for (int k = 0; k < FS; ++k) {
            double l = 0.0;
            for (int pbk = k; pbk < nb; pbk += FS) l += pt[pbk][cw];
            s += l;
        }
        const float v = (float)(s / HW);
        sf[cw >> 1][cw & 1] = v;
        red[2 * ((long)n * C + cg * CG) + cw] = v;
    }
    __syncthreads();
    float mg[8], mgx[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { mg[k] = sf[h * 8 + k][0]; mgx[k] = sf[h * 8 + k][1]; }

    const float qs = F8 ? *q8.q : 1.f;
    float amx = 0.f;
    uint8_t* qb = F8 ? q8.p + pb * q8.ld + q8.off + cg * CG : nullptr;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        // opaque to the optimiser: xhat and g are recomputed from the 8 raw registers, not kept
        // from the first phase as 16 floats per item (there is no room for them)
        asm volatile("" : "+v"(xr[u].x), "+v"(xr[u].y), "+v"(xr[u].z), "+v"(xr[u].w));
        asm volatile("" : "+v"(gr[u].x), "+v"(gr[u].y), "+v"(gr[u].z), "+v"(gr[u].w));
        const uint32_t p = r0 + u * RP;
        if ((int)p >= r1) break;
        float xv[8], gv[8], o[8];
        bf8f(xr[u], xv);
        bf8f(gr[u], gv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            // rstd * (g - mg - xh * mgx) as rows8_kernel<2> compiles it: two fused steps
            const float xh = (xv[k] - mean[k]) * rstd[k];
            const float f = xh > 0.f ? 1.f : neg;
            o[k] = rstd[k] * __builtin_fmaf(-xh, mgx[k], __builtin_fmaf(gv[k], f, -mg[k]));
        }
        uint4 w;
        w.x = pk_bf16(o[0], o[1]);
        w.y = pk_bf16(o[2], o[3]);
        w.z = pk_bf16(o[4], o[5]);
        w.w = pk_bf16(o[6], o[7]);
        *(uint4*)(ob + (p * (uint32_t)lddx + h8)) = w;
        if constexpr (F8) {
            float vb[8];
            bf8f(w, vb);
#pragma unroll
            for (int k = 0; k < 8; ++k) amx = fmaxf(amx, fabsf(vb[k]));
            *(uint2*)(qb + (p * (uint32_t)q8.ld + h8)) = pack8_fp8(vb, qs);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (F8) fp8_block_amax(amx, q8.amax, blockIdx.x);
}

// The reduce pass's partition at (N, HW, C): the very grid launch_rows<1> launches, nb blocks
// of `rows` rows, RP chains each.  False when a chain is longer than OP_MAXU pixels or the
// chains of the group's octets outnumber OP_MAXNT threads (batches of several hundred images,
// C >= 2048).
struct OnepassPlan {
    RowGrid g;
    int chain, threads;
};
bool onepass_plan(int N, int HW, int C, OnepassPlan* pl) {
    pl->g = pass_grid(1, N, HW, C, V);
    pl->chain = irgan_cdiv(pl->g.rows, pl->g.RP);
    pl->threads = pl->g.nb * pl->g.RP * (OP_CG / 8);
    return pl->chain <= OP_MAXU && pl->threads <= OP_MAXNT && pl->g.nb <= IN_PARTS;
}

// legal: all-bf16 callers only (the entry points take no dtypes), the slice fits the
// registers in the reduce pass's partition, whole channel groups, 16-byte lanes
bool onepass_ok(int N, int HW, int C, std::initializer_list<int> lds) {
    if (N < 0 || HW < 0 || C < 0 || C % OP_CG || (long)HW * OP_CG > OP_CAP) return false;
    for (int l : lds)
        if (l % 8 || l < 0 || (long)HW * l >= (1L << 30)) return false;   // 32-bit lane offsets
    OnepassPlan pl;
    return (long)N * HW * C <= 0 || onepass_plan(N, HW, C, &pl);
}

// the instance with NT >= the plan's threads (128 / 256 / 512) and U >= its chain (1 .. 16)
template <bool F8, int NT, int U>
void onepass_launch(const OnepassPlan& pl, hipStream_t st, const RowArgs& a) {
    in_bwd_onepass_kernel<F8, NT, OP_CG, U><<<a.N * (a.C / OP_CG), NT, 0, st>>>(
        bfp(a.X), a.X.ld, a.X.off, bfp(a.DY), a.DY.ld, a.DY.off, a.act, a.mr, a.red_out, (bf16_t*)a.DX.p, a.DX.ld,
        a.DX.off, a.HW, a.C, irgan_xcd_swz(), pl.g.nb, pl.g.rows, pl.g.RP, a.q8);
}
template <bool F8, int NT>
void onepass_nt(const OnepassPlan& pl, hipStream_t st, const RowArgs& a) {
    if (pl.chain <= 1) onepass_launch<F8, NT, 1>(pl, st, a);
    else if (pl.chain <= 2) onepass_launch<F8, NT, 2>(pl, st, a);
    else if (pl.chain <= 4) onepass_launch<F8, NT, 4>(pl, st, a);
    else if (pl.chain <= 8) onepass_launch<F8, NT, 8>(pl, st, a);
    else onepass_launch<F8, NT, 16>(pl, st, a);
}
template <bool F8>
void onepass_go(const RowArgs& a, hipStream_t st) {
    OnepassPlan pl;
    onepass_plan(a.N, a.HW, a.C, &pl);
    if (pl.threads <= 128) onepass_nt<F8, 128>(pl, st, a);
    else if (pl.threads <= 256) onepass_nt<F8, 256>(pl, st, a);
    else onepass_nt<F8, 512>(pl, st, a);
}

// the forward apply as rows8_kernel<4> (all bf16, 8-channel vectors, no xhat; the residual in
// a.DY), grid as the other row passes; a.q8.p: also the fp8 copy of y (irgan_in_apply_fp8) --
// without the amax record when a.q8.amax is null, and then alone when a.DX.p is null too
void apply_rows(const RowArgs& a, hipStream_t st) {
    const int key = a.DY.p || a.q8.p ? 5 : 4;  // 5: apply + residual, or with the fp8 copy
    const RowGrid g = pass_grid(key, a.N, a.HW, a.C, V);
    if (!a.q8.p) rows8_go<4, false>(key, g, st, a);
    else if (a.q8.amax && a.DX.p) rows8_go<4, true>(key, g, st, a);
    else if (a.DX.p) rows8_go<4, true, false, true>(key, g, st, a);
    else rows8_go<4, true, false, false>(key, g, st, a);
}

// db[c] += sum of the nb partials' .x, in lane_combine's order (deterministic)
__global__ __launch_bounds__(256) void colsum_finalize_kernel(const float2* __restrict__ part, float* __restrict__ db,
                                                              int nb, int C) {
    __shared__ double sm[1][FS][FC];
    const int cl = threadIdx.x % FC, sub = threadIdx.x / FC, c = blockIdx.x * FC + cl;
    double t[1];
    lane_combine<1>(nb, c < C, sub, cl, sm, t, [&](int b, double* v) { v[0] += part[(long)b * C + c].x; });
    if (sub != 0 || c >= C) return;
    db[c] += (float)t[0];
}

// the arguments the backward entry points share; false: IRGAN_EINVAL
bool bwd_args(RowArgs* a, const void* dy, int dy_dtype, int lddy, int dyoff, const void* dy2, int dy2_dtype,
              int lddy2, int dy2off, const void* x, int x_dtype, int ldx, int xoff, int act, int N, int HW, int C,
              const float* mr) {
    if (!dy || !x || !mr || !dt_ok(dy_dtype) || !dt_ok(x_dtype) || (dy2 && !dt_ok(dy2_dtype)) || !act_ok(act) ||
        !slice_ok(C, lddy, dyoff) || !slice_ok(C, ldx, xoff) || (dy2 && !slice_ok(C, lddy2, dy2off)))
        return false;
    a->X = {x, x_dtype, ldx, xoff};
    a->DY = {dy, dy_dtype, lddy, dyoff};
    a->DY2 = {dy2, dy2_dtype, lddy2, dy2off};
    a->act = act; a->mr = mr;
    a->N = N; a->HW = HW; a->C = C;
    return true;
}

// the slices of an all-bf16 backward (the one-pass and fp8 entry points take no dtypes)
RowArgs bf16_bwd(const void* dy, int lddy, int dyoff, const void* x, int ldx, int xoff, int act, int N, int HW, int C,
                 const float* mr, void* dx, int lddx, int dxoff) {
    RowArgs a{};
    a.X = {x, IRGAN_BF16, ldx, xoff};
    a.DY = {dy, IRGAN_BF16, lddy, dyoff};
    a.act = act; a.mr = mr;
    a.DX = {dx, IRGAN_BF16, lddx, dxoff};
    a.N = N; a.HW = HW; a.C = C;
    return a;
}

}  // namespace

// Argument checks of the entry points (as batchnorm.hip's): empty work returns 0 before them;
// a null required pointer, an unknown dtype or activation, or a slice that leaves its rows is
// IRGAN_EINVAL and launches nothing.

extern "C" int irgan_in_stats(const void* x, int32_t dtype, int32_t N, int32_t HW, int32_t C, int32_t ld,
                              int32_t off, double* work, float* mr, irgan_stream_t s) {
    hipStream_t st = (hipStream_t)s;
    if ((long)N * HW * C <= 0) return 0;
    if (!x || !work || !mr || !dt_ok(dtype) || !slice_ok(C, ld, off)) return IRGAN_EINVAL;
    RowArgs a{};
    a.X = {x, dtype, ld, off};
    a.N = N; a.HW = HW; a.C = C;
    a.part = (float2*)work;
    const int nb = launch_rows<0>(a, vec_ok(C, {ld, off}), st);
    finalize_kernel<<<dim3(irgan_cdiv(C, FC), N), 256, 0, st>>>((const float2*)work, mr, N, C, nb, HW, 0);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_in_finalize(const void* part, int32_t N, int32_t HW, int32_t C, int32_t nb, float* mr,
                                 irgan_stream_t s) {
    if ((long)N * HW * C <= 0) return 0;
    if (!part || !mr || nb < 1 || nb > IRGAN_IN_PARTS) return IRGAN_EINVAL;
    finalize_kernel<<<dim3(irgan_cdiv(C, FC), N), 256, 0, (hipStream_t)s>>>((const float2*)part, mr, N, C, nb, HW, 0);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_in_apply(const void* x, int32_t dtype, int32_t N, int32_t HW, int32_t C, int32_t ldx,
                              int32_t xoff, const float* mr, int32_t act, const void* res, int32_t ldr, int32_t roff,
                              void* y, int32_t ldy, int32_t yoff, void* xhat, irgan_stream_t s) {
    if ((long)N * HW * C <= 0) return 0;
    if (!x || !mr || !y || !dt_ok(dtype) || !act_ok(act) || !slice_ok(C, ldx, xoff) || !slice_ok(C, ldy, yoff) ||
        (res && !slice_ok(C, ldr, roff)))
        return IRGAN_EINVAL;
    const bool vec = vec_ok(C, {ldx, xoff, ldy, yoff}) && (!res || vec_ok(C, {ldr, roff}));
    const Slice X{x, dtype, ldx, xoff}, R{res, dtype, ldr, roff};
    if (vec && dtype == IRGAN_BF16 && !xhat) {
        RowArgs a{};
        a.X = X; a.DY = R; a.act = act; a.mr = mr;
        a.DX = {y, dtype, ldy, yoff};
        a.N = N; a.HW = HW; a.C = C;
        apply_rows(a, (hipStream_t)s);
        IRGAN_LAUNCH_CHECK();
        return 0;
    }
    const long total = (long)N * HW * (C / (vec ? V : 1));
    const int blocks = (int)std::min<long>((total + TPB - 1) / TPB, 16384);
    if (vec)
        apply_kernel<V><<<blocks, TPB, 0, (hipStream_t)s>>>(X, HW, C, mr, act, R, y, ldy, yoff, xhat, total);
    else
        apply_kernel<1><<<blocks, TPB, 0, (hipStream_t)s>>>(X, HW, C, mr, act, R, y, ldy, yoff, xhat, total);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_in_bwd_reduce(const void* dy, int32_t dy_dtype, int32_t lddy, int32_t dyoff, const void* dy2,
                                   int32_t dy2_dtype, int32_t lddy2, int32_t dy2off, const void* x, int32_t x_dtype,
                                   int32_t ldx, int32_t xoff, int32_t act, int32_t N, int32_t HW, int32_t C,
                                   const float* mr, double* work, float* red, irgan_stream_t s) {
    hipStream_t st = (hipStream_t)s;
    if ((long)N * HW * C <= 0) return 0;
    RowArgs a{};
    if (!work || !red ||
        !bwd_args(&a, dy, dy_dtype, lddy, dyoff, dy2, dy2_dtype, lddy2, dy2off, x, x_dtype, ldx, xoff, act, N, HW, C,
                  mr))
        return IRGAN_EINVAL;
    a.part = (float2*)work;
    const bool vec = vec_ok(C, {lddy, dyoff, ldx, xoff}) && (!dy2 || vec_ok(C, {lddy2, dy2off}));
    const int nb = launch_rows<1>(a, vec, st);
    finalize_kernel<<<dim3(irgan_cdiv(C, FC), N), 256, 0, st>>>((const float2*)work, red, N, C, nb, HW, 1);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

// irgan_in_bwd_reduce over a gradient that is not stored: rows8_adjoint_reduce_kernel on the reduce
// pass's own grid, then its finalize (resample.hip: irgan_sep_resample_in_bwd_reduce, which checks
// the arguments -- all bf16, 8-channel vectors, at most 2 taps per axis; not exported)
int in_bwd_reduce_adjoint_launch(const void* dy, int lddy, int dyoff, int Hin, int Win, const int* ty, const float* wy,
                                 int Ty, const int* tx, const float* wx, int Tx, const void* z, int ldz, int zoff,
                                 int act, int N, int Hout, int Wout, int C, const float* mr, double* work, float* red,
                                 hipStream_t st) {
    const int HW = Hout * Wout;
    const RowGrid g = pass_grid(1, N, HW, C, V);
    const int NR = (g.rows + Wout - 1) / Wout + 1;   // output rows a block's g.rows pixels can lie in
    const size_t sh = (size_t)(2 * Wout + 2 * NR) * 8;
    if (Ty > 2 || Tx > 2 || C % V || g.nb > IN_PARTS || sh > 40 * 1024) return IRGAN_EINVAL;
#define ADJ(UV)                                                                                                    \
    rows8_adjoint_reduce_kernel<UV><<<dim3(g.nb, N), TPB, sh, st>>>(                                               \
        (const bf16_t*)z, ldz, zoff, (const bf16_t*)dy, lddy, dyoff, Hin, Win, Wout, ty, wy, Ty, tx, wx, Tx, act, mr, \
        HW, C, g.rows, NR, (float2*)work)
    if (irgan_cdiv(g.rows, g.RP) <= 1) ADJ(1);
    else ADJ(2);
#undef ADJ
    finalize_kernel<<<dim3(irgan_cdiv(C, FC), N), 256, 0, st>>>((const float2*)work, red, N, C, g.nb, HW, 1);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_in_bwd_apply(const void* dy, int32_t dy_dtype, int32_t lddy, int32_t dyoff, const void* dy2,
                                  int32_t dy2_dtype, int32_t lddy2, int32_t dy2off, const void* x, int32_t x_dtype,
                                  int32_t ldx, int32_t xoff, int32_t act, int32_t N, int32_t HW, int32_t C,
                                  const float* mr, const float* red, void* dx, int32_t dx_dtype, int32_t lddx,
                                  int32_t dxoff, float* db, irgan_stream_t s) {
    if ((long)N * HW * C <= 0) return 0;
    RowArgs a{};
    if (!red || !dx || !dt_ok(dx_dtype) || !slice_ok(C, lddx, dxoff) ||
        !bwd_args(&a, dy, dy_dtype, lddy, dyoff, dy2, dy2_dtype, lddy2, dy2off, x, x_dtype, ldx, xoff, act, N, HW, C,
                  mr))
        return IRGAN_EINVAL;
    a.red = red;
    a.DX = {dx, dx_dtype, lddx, dxoff};
    a.db = db;
    const bool vec = vec_ok(C, {lddy, dyoff, ldx, xoff, lddx, dxoff}) && (!dy2 || vec_ok(C, {lddy2, dy2off}));
    launch_rows<2>(a, vec, (hipStream_t)s);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_in_bwd_onepass(const void* dy, int32_t dy_dtype, int32_t lddy, int32_t dyoff, const void* dy2,
                                    int32_t dy2_dtype, int32_t lddy2, int32_t dy2off, const void* x, int32_t x_dtype,
                                    int32_t ldx, int32_t xoff, int32_t act, int32_t N, int32_t HW, int32_t C,
                                    const float* mr, float* red, void* dx, int32_t dx_dtype, int32_t lddx,
                                    int32_t dxoff, irgan_stream_t s) {
    (void)dy2_dtype; (void)lddy2; (void)dy2off;
    if (!dy || !x || !mr || !red || !dx) return IRGAN_EINVAL;
    if (dy2 || dy_dtype != IRGAN_BF16 || x_dtype != IRGAN_BF16 || dx_dtype != IRGAN_BF16 ||
        !onepass_ok(N, HW, C, {lddy, dyoff, ldx, xoff, lddx, dxoff}))
        return IRGAN_EUNSUPPORTED;
    if ((long)N * HW * C <= 0) return 0;
    RowArgs a = bf16_bwd(dy, lddy, dyoff, x, ldx, xoff, act, N, HW, C, mr, dx, lddx, dxoff);
    a.red_out = red;
    onepass_go<false>(a, (hipStream_t)s);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_in_bwd_onepass_fp8(const void* dy, int32_t lddy, int32_t dyoff, const void* dy2, int32_t lddy2,
                                        int32_t dy2off, const void* x, int32_t ldx, int32_t xoff, int32_t act,
                                        int32_t N, int32_t HW, int32_t C, const float* mr, float* red, void* dx,
                                        int32_t lddx, int32_t dxoff, void* y8, int32_t ld8, int32_t off8,
                                        const float* q, uint32_t* amax, irgan_stream_t s) {
    (void)lddy2; (void)dy2off;
    if (!dy || !x || !mr || !red || !dx || !y8 || !q || !amax) return IRGAN_EINVAL;
    if (dy2 || !onepass_ok(N, HW, C, {lddy, dyoff, ldx, xoff, lddx, dxoff, ld8, off8})) return IRGAN_EUNSUPPORTED;
    if ((long)N * HW * C <= 0) return 0;
    RowArgs a = bf16_bwd(dy, lddy, dyoff, x, ldx, xoff, act, N, HW, C, mr, dx, lddx, dxoff);
    a.red_out = red;
    a.q8 = {(uint8_t*)y8, ld8, off8, q, amax};
    onepass_go<true>(a, (hipStream_t)s);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

// Bias gradient (sum over the P rows of each channel).  The rows are split into S <= 16
// equal segments run as S "images" of launch_rows (S x <= IN_PARTS block partials: with one
// image a single row of <= IN_PARTS blocks streamed the D input layer's 67 MB gradient at
// ~1.6 TB/s), then summed in a fixed order (no atomics).  work: 16 * IN_PARTS * C doubles.
extern "C" int irgan_channel_sum(const void* g, int32_t dtype, int32_t P, int32_t C, int32_t ld, int32_t off,
                                 float* db, double* work, irgan_stream_t s) {
    if (P <= 0 || C <= 0) return 0;
    if (!g || !db || !work || !dt_ok(dtype) || !slice_ok(C, ld, off)) return IRGAN_EINVAL;
    hipStream_t st = (hipStream_t)s;
    int S = 16;
    while (S > 1 && (P % S || P / S < 4096)) S >>= 1;
    RowArgs a{};
    a.X = {g, dtype, ld, off};
    a.N = S; a.HW = P / S; a.C = C;
    a.part = (float2*)work;
    const int nb = launch_rows<0>(a, vec_ok(C, {ld, off}), st);
    colsum_finalize_kernel<<<irgan_cdiv(C, FC), 256, 0, st>>>((const float2*)work, db, S * nb, C);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

// irgan_in_apply / irgan_in_bwd_apply that also write the fp8 copy of their bf16
// output (Q8 above): the producers of the fp8 path's ResnetBlock conv operands.
extern "C" int irgan_in_apply_fp8(const void* x, int32_t N, int32_t HW, int32_t C, int32_t ldx, int32_t xoff,
                                  const float* mr, int32_t act, const void* res, int32_t ldr, int32_t roff, void* y,
                                  int32_t ldy, int32_t yoff, void* y8, int32_t ld8, int32_t off8, const float* q,
                                  uint32_t* amax, irgan_stream_t s) {
    // amax NULL: nothing is recorded; y NULL: y8 alone -- only without the record (the eval-mode
    // forward's call) and without a residual (the sum is the next block's residual, needed in bf16)
    if (!x || !mr || !y8 || !q || (!y && (res || amax))) return IRGAN_EINVAL;
    if (!y) ldy = ld8, yoff = off8;   // unused: pass the checks below
    if (!vec_ok(C, {ldx, xoff, ldy, yoff, ld8, off8}) || (res && !vec_ok(C, {ldr, roff}))) return IRGAN_EUNSUPPORTED;
    if ((long)N * HW * C <= 0) return 0;
    RowArgs a{};
    a.X = {x, IRGAN_BF16, ldx, xoff};
    a.DY = {res, IRGAN_BF16, ldr, roff};
    a.act = act; a.mr = mr;
    a.DX = {y, IRGAN_BF16, ldy, yoff};
    a.N = N; a.HW = HW; a.C = C;
    a.q8 = {(uint8_t*)y8, ld8, off8, q, amax};
    apply_rows(a, (hipStream_t)s);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_in_bwd_apply_fp8(const void* dy, int32_t lddy, int32_t dyoff, const void* dy2, int32_t lddy2,
                                      int32_t dy2off, const void* x, int32_t ldx, int32_t xoff, int32_t act, int32_t N,
                                      int32_t HW, int32_t C, const float* mr, const float* red, void* dx, int32_t lddx,
                                      int32_t dxoff, void* y8, int32_t ld8, int32_t off8, const float* q,
                                      uint32_t* amax, irgan_stream_t s) {
    if (!dy || !x || !mr || !red || !dx || !y8 || !q || !amax) return IRGAN_EINVAL;
    if ((long)N * HW * C <= 0) return 0;
    // all bf16 in 8-channel vectors and no db: what launch_rows<2> needs to take rows8_kernel's fp8 instance
    const bool vec =
        vec_ok(C, {lddy, dyoff, ldx, xoff, lddx, dxoff, ld8, off8}) && (!dy2 || vec_ok(C, {lddy2, dy2off}));
    if (!vec) return IRGAN_EUNSUPPORTED;
    RowArgs a = bf16_bwd(dy, lddy, dyoff, x, ldx, xoff, act, N, HW, C, mr, dx, lddx, dxoff);
    a.red = red;
    a.DY2 = {dy2, IRGAN_BF16, lddy2, dy2off};
    a.q8 = {(uint8_t*)y8, ld8, off8, q, amax};
    launch_rows<2>(a, true, (hipStream_t)s);
    IRGAN_LAUNCH_CHECK();
    return 0;
}
