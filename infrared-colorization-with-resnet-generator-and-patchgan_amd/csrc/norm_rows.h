// The row-pass toolkit of the normalisation kernels (norm.hip: InstanceNorm and the channel
// sums, batchnorm.hip: BatchNorm2d).  A row pass streams an NHWC slice: a block of TPB threads
// covers a run of rows of one image, CL lanes across the channels (VW = 8 or 1 channels each),
// RP rows in parallel; a thread adds its rows r0 + rl, r0 + rl + RP, ... in order (a chain),
// the block combines the RP chains of a channel (block_reduce) into one partial per (block,
// channel), and a finalize launch adds the partials in fp64 (lane_combine).
//
// THE REDUCTION ORDER IS DEFINED HERE, once: the results of both files are reproducible bit
// for bit because every sum is grouped by row_grid (which rows meet in a chain, a block),
// block_reduce (how the chains of a block meet) and lane_combine (how the blocks meet).
// norm.hip's one-pass backward re-enacts the same three groupings in LDS.
#pragma once
#include "common.h"

#include <algorithm>
#include <initializer_list>

namespace {

constexpr int TPB = 256;
constexpr int V = 8;              // channels per thread of the vector form
constexpr int FC = 8, FS = 32;    // finalize block: FC channels x FS partial lanes

// channels off .. off + C of rows of ld elements of type dt; OSlice: one that is written
struct Slice {
    const void* p;
    int dt, ld, off;
};
struct OSlice {
    void* p;
    int dt, ld, off;
};

// ---- host side: argument checks and the grid -----------------------------------------

inline bool dt_ok(int dt) { return dt == IRGAN_F32 || dt == IRGAN_BF16; }
inline bool act_ok(int act) { return act >= IRGAN_ACT_NONE && act <= IRGAN_ACT_LRELU; }
// channels off .. off + C of rows of ld elements
inline bool slice_ok(int C, int ld, int off) { return off >= 0 && (long)off + C <= ld; }

// the 8-channel form: whole octets, 16-byte aligned rows and offsets
inline bool vec_ok(int C, std::initializer_list<int> lds) {
    if (C % V) return false;
    for (int l : lds)
        if (l % V) return false;
    return true;
}

// Grid of a row pass over N images of HW rows: ~4096 blocks in all, >= rpt rows per thread,
// <= cap blocks (partials) per image; nb blocks of `rows` rows, RP chains each.
struct RowGrid {
    int nb, rows, RP;
};
inline RowGrid row_grid(int N, long HW, int C, int VW, long rpt, long cap) {
    int cl = (C + VW - 1) / VW;
    if (cl > TPB) cl = TPB;
    RowGrid g;
    g.RP = TPB / cl;
    long nb = (4096 + N - 1) / (N > 0 ? N : 1);
    nb = std::min(nb, (HW + rpt * g.RP - 1) / (rpt * g.RP));
    nb = std::max(1L, std::min(nb, cap));
    g.rows = irgan_cdiv(HW, nb);
    g.nb = irgan_cdiv(HW, g.rows);
    return g;
}

// ---- device side ---------------------------------------------------------------------

// 8 bf16 (one 16-byte load, still raw) -> 8 floats: for the kernels that issue a batch of raw
// loads before converting any (rows8_kernel, the one-pass backward)
IRGAN_HD void bf8f(const uint4 u, float* o) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        o[2 * k] = __uint_as_float(w[k] << 16);
        o[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
    }
}

// VW consecutive elements at index i through a dtype code, as floats.  The bf16 branch is
// bf8f's conversion, written out: through the call bn_apply_kernel<8> and the BatchNorm row
// passes allocate differently (profiles/norm_rows_refactor.txt)
template <int VW>
IRGAN_HD void ldw(const void* p, int dt, long i, float* o) {
    if constexpr (VW == 8) {
        if (dt == IRGAN_BF16) {
            const uint4 u = *(const uint4*)((const bf16_t*)p + i);
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[2 * k] = __uint_as_float(w[k] << 16);
                o[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
            }
        } else {
            const float4 a = *(const float4*)((const float*)p + i), b = *(const float4*)((const float*)p + i + 4);
            o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
        }
    } else {
        o[0] = ldv(p, dt, i);
    }
}
template <int VW>
IRGAN_HD void stw(void* p, int dt, long i, const float* v) {
    if constexpr (VW == 8) {
        if (dt == IRGAN_BF16) {
            uint4 u;
            u.x = pk_bf16(v[0], v[1]);
            u.y = pk_bf16(v[2], v[3]);
            u.z = pk_bf16(v[4], v[5]);
            u.w = pk_bf16(v[6], v[7]);
            *(uint4*)((bf16_t*)p + i) = u;
        } else {
            *(float4*)((float*)p + i) = make_float4(v[0], v[1], v[2], v[3]);
            *(float4*)((float*)p + i + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
    } else {
        stv(p, dt, i, v[0]);
    }
}

// the activation that follows a norm, and its derivative (h: the activation's input)
IRGAN_HD float act_fwd(float h, int act) {
    if (act == IRGAN_ACT_RELU) return h > 0.f ? h : 0.f;
    if (act == IRGAN_ACT_LRELU) return h > 0.f ? h : 0.2f * h;
    return h;
}
IRGAN_HD float act_grad(float h, int act) {
    if (act == IRGAN_ACT_RELU) return h > 0.f ? 1.f : 0.f;
    if (act == IRGAN_ACT_LRELU) return h > 0.f ? 1.f : 0.2f;
    return 1.f;
}

// block layout: CL lanes per row (VW channels each), RP rows in parallel
struct Lay {
    int CL, RP, cl, rl;
    __device__ Lay(int C, int VW) {
        CL = (C + VW - 1) / VW;
        if (CL > TPB) CL = TPB;
        RP = TPB / CL;
        cl = threadIdx.x % CL;
        rl = threadIdx.x / CL;
    }
    // the same four values, computed by the caller (batchnorm.hip's kernels, which spell the
    // formula above out in their bodies: keep the two equal)
    __device__ Lay(int CL_, int RP_, int cl_, int rl_) : CL(CL_), RP(RP_), cl(cl_), rl(rl_) {}
};

// How block_reduce combines the RP chains of a channel.  The order is the result.
//   ROWS_TREE:   a butterfly over the rows inside each wave, then the TPB / 64 waves in
//                order; legal only when the channel lanes divide a wave (rows_tree_ok)
//   ROWS_CHAINS: the RP chains in order
enum RowOrder { ROWS_TREE, ROWS_CHAINS };
IRGAN_HD bool rows_tree_ok(int CL) { return CL <= 64 && (64 % CL) == 0; }
// InstanceNorm's choice (norm.hip): the tree wherever it is legal.  BatchNorm's passes always
// take ROWS_CHAINS.
IRGAN_HD RowOrder in_row_order(int CL) { return rows_tree_ok(CL) ? ROWS_TREE : ROWS_CHAINS; }

// Block-wide per-channel sums of the accumulator pairs (a0, a1) (VW channels per thread) of
// channel block cb; c = cb + L.cl * VW, on = this thread holds rows of valid channels.  The
// thread that owns channels cc .. cc + VW - 1 of the block gets emit(cc, k, total a0, total a1)
// for each of them.  Every thread of the block calls it (barriers); s0, s1: TPB * VW values of
// LDS each.
template <typename T, int VW, typename Emit>
IRGAN_HD void block_reduce(T* a0, T* a1, const Lay& L, RowOrder order, bool on, int cb, int c, int C, T* s0, T* s1,
                           Emit emit) {
    if (order == ROWS_TREE) {
        // rows of one wave share a lane's channels every CL lanes: butterfly over them, then
        // one LDS slot per (wave, channel lane)
        for (int o = L.CL; o < 64; o <<= 1) {
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                a0[k] += __shfl_xor(a0[k], o, 64);
                a1[k] += __shfl_xor(a1[k], o, 64);
            }
        }
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        if (lane < L.CL) {
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                s0[(wv * L.CL + lane) * VW + k] = a0[k];
                s1[(wv * L.CL + lane) * VW + k] = a1[k];
            }
        }
        __syncthreads();
        if (threadIdx.x < L.CL && cb + threadIdx.x * VW < C) {
            const int cc = cb + threadIdx.x * VW;
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                T t0 = 0, t1 = 0;
                for (int j = 0; j < TPB / 64; ++j) {
                    t0 += s0[(j * L.CL + threadIdx.x) * VW + k];
                    t1 += s1[(j * L.CL + threadIdx.x) * VW + k];
                }
                emit(cc, k, t0, t1);
            }
        }
        __syncthreads();
        return;
    }
#pragma unroll
    for (int k = 0; k < VW; ++k) {
        s0[threadIdx.x * VW + k] = a0[k];
        s1[threadIdx.x * VW + k] = a1[k];
    }
    __syncthreads();
    if (on && L.rl == 0) {   // the first row of lanes sums the RP rows in order
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            T t0 = 0, t1 = 0;
            for (int j = 0; j < L.RP; ++j) {
                t0 += s0[(j * L.CL + L.cl) * VW + k];
                t1 += s1[(j * L.CL + L.cl) * VW + k];
            }
            emit(c, k, t0, t1);
        }
    }
    __syncthreads();
}

// The fixed-order fp64 combine of cnt partials of NV values each, in a finalize block of FC
// channels x FS partial lanes (cl = threadIdx.x % FC, sub = threadIdx.x / FC): lane sub adds
// partials sub, sub + FS, ... through add(j, v) (at most cnt / FS dependent loads: these
// launches are latency-bound, so the lanes are many and the channel groups narrow), then the
// FS lanes of a channel meet in LDS and lane 0 adds them in order.  v[] holds the sums where
// sub == 0.  Every thread of the block calls it; `in` = the thread's channel exists.
template <int NV, typename Add>
IRGAN_HD void lane_combine(int cnt, bool in, int sub, int cl, double (*sm)[FS][FC], double* v, Add add) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = 0.0;
    if (in)
        for (int j = sub; j < cnt; j += FS) add(j, v);
#pragma unroll
    for (int i = 0; i < NV; ++i) sm[i][sub][cl] = v[i];
    __syncthreads();
    if (sub != 0) return;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = 0.0;
        for (int k = 0; k < FS; ++k) v[i] += sm[i][k][cl];
    }
}

}  // namespace
