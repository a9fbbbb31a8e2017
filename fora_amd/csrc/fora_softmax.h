// fora_softmax.h -- the kernels of ROW SOFTMAX (fora_hip_sparse_softmax, fora_hip_sparse_softmax_bwd; the contract is in
// include/fora_hip.h): softmax inside every held row, and its gradient, every bit defined.
//   forward   x_e = (double)scores[e] * scale;  m = the row's largest x;  p_e = exp_def(x_e - m) (fora_softmax_exp.h);
//             S = the row's sum of p in the order below;  y_e = p_e / S.  A NaN entry, m = +inf or m = -inf: the row is NaN.
//   backward  t_e = (double)y_e * (double)g_e;  D = the row's sum of t in the same order;  dx_e = ((g_e - D) * y_e) * scale.
//   the sum   a row is cut every PROP_SEG = 256 entries.  In a segment q_l, l = 0 .. 63, adds the terms at the positions
//             j == l (mod 64) in ascending j from +0.0; then q_l = q_l + q_{l+o} for l < o, o = 32 .. 1; P_s = q_0.  The row's
//             sum is P_0, then + P_s for s = 1, 2, ... in order.
// One wave owns a segment: lane l holds the terms l, l + 64, l + 128, l + 192 in registers, so q_l is a lane's own sum and the
// tree is six exchanges.  Two paths, the same bits:
//   short  a row of at most `softmax_short` (<= 256) entries is one segment: one wave reads it once, takes the maximum, sums,
//          divides and writes it once.  No LDS, no partial in memory; BLOCK / 64 rows per workgroup.
//   long   the segments of the longer rows, one wave each, in three launches (two backward): the segment maxima; the segment
//          sums under the row's maximum; the division by the row's sum.  A segment of this list says where its row's segments
//          start in the list and how many they are, so a wave reads the row's few partials itself: the maximum over them (any
//          order gives the same bits), the sum one after the other.  A row of 26 000 entries is 103 waves, not one.
// The work lists are PropSeg lists (fora_prop_plan.h) split by the host into the two paths (fora_softmax_plan.h).
// Nothing is fused: the file is compiled with -ffp-contract=off and every kernel says so again itself.
#pragma once
#include "fora_kernels.h" // BLOCK
#include "fora_softmax_exp.h"
#include "fora_softmax_plan.h" // PropSeg and the two lists

namespace fora {

constexpr uint32_t SMAX_PER_LANE = PROP_SEG / 64; // entries of a segment that one lane holds
static_assert(PROP_SEG % 64 == 0, "a lane holds whole strides of a segment");

__device__ __forceinline__ double smax_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ double smax_neg_inf() { return __longlong_as_double((long long)0xFFF0000000000000ull); }
__device__ __forceinline__ bool smax_is_inf(double m) { return (__double_as_longlong(m) & 0x7FFFFFFFFFFFFFFFll) == 0x7FF0000000000000ll; }

// the contract's tree over the 64 q_l of a wave; every lane returns q_0.  Lane l < o adds q_l + q_{l^o} = q_l + q_{l+o}; what
// the lanes l >= o compute is never read by a lane below the next o.
__device__ __forceinline__ double smax_tree(double q) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 32; o; o >>= 1) q = q + __shfl_xor(q, o, 64);
    return __shfl(q, 0, 64);
}
// the largest of the wave's m (none is NaN); +0.0 against -0.0 may go either way, which changes no output bit
__device__ __forceinline__ double smax_wave_max(double m) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double v = __shfl_xor(m, o, 64);
        m = v > m ? v : m;
    }
    return m;
}
// x of the segment's entries this lane holds, and their maximum with a NaN read as +inf (either makes the row NaN)
template <typename TS>
__device__ __forceinline__ double smax_load_x(const PropSeg &sg, uint32_t lane, const TS *scores, double scale, double (&x)[SMAX_PER_LANE]) {
#pragma clang fp contract(off)
    double m = smax_neg_inf();
#pragma unroll
    for (uint32_t j = 0; j < SMAX_PER_LANE; j++) {
        const uint32_t k = lane + 64u * j;
        x[j] = smax_neg_inf();
        if (k < sg.len) {
            x[j] = (double)scores[sg.first + k] * scale;
            const double v = x[j] != x[j] ? -smax_neg_inf() : x[j];
            m = v > m ? v : m;
        }
    }
    return m;
}
// P_s of p = exp_def(x - m) over the lane's entries; p is left in x
__device__ __forceinline__ double smax_exp_sum(const PropSeg &sg, uint32_t lane, double m, double (&x)[SMAX_PER_LANE]) {
#pragma clang fp contract(off)
    double q = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < SMAX_PER_LANE; j++) {
        if (lane + 64u * j < sg.len) {
            x[j] = exp_def(x[j] - m);
            q = q + x[j];
        }
    }
    return smax_tree(q);
}
__device__ __forceinline__ void smax_store(const PropSeg &sg, uint32_t lane, const double (&v)[SMAX_PER_LANE], float *out32, double *out64) {
#pragma unroll
    for (uint32_t j = 0; j < SMAX_PER_LANE; j++) {
        const uint32_t k = lane + 64u * j;
        if (k < sg.len) {
            if (out64) out64[sg.first + k] = v[j];
            if (out32) out32[sg.first + k] = (float)v[j];
        }
    }
}
// the row's maximum from the maxima of its segments (long list)
__device__ __forceinline__ double smax_row_max(const PropSeg &sg, uint32_t lane, const double *seg_max) {
    double m = smax_neg_inf();
    for (uint32_t s = lane; s < sg.pad_; s += 64u) {
        const double v = seg_max[sg.slot + s];
        m = v > m ? v : m;
    }
    return smax_wave_max(m);
}
// the row's sum from the sums of its segments, one after the other (long list); the same loads on every lane
__device__ __forceinline__ double smax_row_sum(const PropSeg &sg, const double *part) {
#pragma clang fp contract(off)
    double S = part[sg.slot];
    for (uint32_t s = 1; s < sg.pad_; s++) S = S + part[sg.slot + s];
    return S;
}

#define SMAX_WAVE_PROLOGUE                                                                     \
    const uint32_t lane = threadIdx.x & 63u;                                                   \
    const uint64_t u = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);               \
    if (u >= nseg) return; /* (the whole wave) */                                              \
    const PropSeg sg = segs[u];

// ---- forward.  grid = ceil(nseg / (BLOCK / 64)) workgroups of BLOCK threads in every kernel: wave u owns segment u.
template <typename TS>
__global__ void __launch_bounds__(BLOCK) k_softmax_short(const PropSeg *segs, uint64_t nseg, const TS *scores, double scale, float *out32, double *out64,
                                                         uint32_t *nan_rows) {
#pragma clang fp contract(off)
    SMAX_WAVE_PROLOGUE
    double x[SMAX_PER_LANE];
    const double m = smax_wave_max(smax_load_x(sg, lane, scores, scale, x));
    if (smax_is_inf(m)) { // (the whole wave: a NaN entry, +inf, or nothing above -inf)
#pragma unroll
        for (uint32_t j = 0; j < SMAX_PER_LANE; j++) x[j] = smax_nan();
        smax_store(sg, lane, x, out32, out64);
        if (lane == 0) atomicAdd(nan_rows, 1u);
        return;
    }
    const double S = smax_exp_sum(sg, lane, m, x);
#pragma unroll
    for (uint32_t j = 0; j < SMAX_PER_LANE; j++) x[j] = x[j] / S;
    smax_store(sg, lane, x, out32, out64);
}

template <typename TS>
__global__ void __launch_bounds__(BLOCK) k_softmax_seg_max(const PropSeg *segs, uint64_t nseg, const TS *scores, double scale, double *seg_max) {
#pragma clang fp contract(off)
    SMAX_WAVE_PROLOGUE
    double x[SMAX_PER_LANE];
    const double m = smax_wave_max(smax_load_x(sg, lane, scores, scale, x));
    if (lane == 0) seg_max[u] = m;
}

template <typename TS>
__global__ void __launch_bounds__(BLOCK) k_softmax_seg_sum(const PropSeg *segs, uint64_t nseg, const TS *scores, double scale, const double *seg_max, double *part) {
#pragma clang fp contract(off)
    SMAX_WAVE_PROLOGUE
    const double m = smax_row_max(sg, lane, seg_max);
    if (smax_is_inf(m)) return; // (a NaN row: k_softmax_div writes it and reads no sum)
    double x[SMAX_PER_LANE];
    (void)smax_load_x(sg, lane, scores, scale, x);
    const double P = smax_exp_sum(sg, lane, m, x);
    if (lane == 0) part[u] = P;
}

template <typename TS>
__global__ void __launch_bounds__(BLOCK) k_softmax_div(const PropSeg *segs, uint64_t nseg, const TS *scores, double scale, const double *seg_max, const double *part,
                                                       float *out32, double *out64, uint32_t *nan_rows) {
#pragma clang fp contract(off)
    SMAX_WAVE_PROLOGUE
    const double m = smax_row_max(sg, lane, seg_max);
    double x[SMAX_PER_LANE];
    if (smax_is_inf(m)) {
#pragma unroll
        for (uint32_t j = 0; j < SMAX_PER_LANE; j++) x[j] = smax_nan();
        smax_store(sg, lane, x, out32, out64);
        if (lane == 0 && u == sg.slot) atomicAdd(nan_rows, 1u); // (the row's first segment counts it)
        return;
    }
    const double S = smax_row_sum(sg, part);
    (void)smax_load_x(sg, lane, scores, scale, x);
#pragma unroll
    for (uint32_t j = 0; j < SMAX_PER_LANE; j++) x[j] = exp_def(x[j] - m) / S; // (an entry past the segment: exp_def(-inf) = +0.0, never stored)
    smax_store(sg, lane, x, out32, out64);
}

// ---- backward: the same two paths with t = y * g in place of p and no maximum
template <typename TY, typename TG>
__device__ __forceinline__ double smax_bwd_load(const PropSeg &sg, uint32_t lane, const TY *y, const TG *g, double (&yv)[SMAX_PER_LANE], double (&gv)[SMAX_PER_LANE]) {
#pragma clang fp contract(off)
    double q = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < SMAX_PER_LANE; j++) {
        const uint32_t k = lane + 64u * j;
        yv[j] = gv[j] = 0.0;
        if (k < sg.len) {
            yv[j] = (double)y[sg.first + k];
            gv[j] = (double)g[sg.first + k];
            const double t = yv[j] * gv[j];
            q = q + t;
        }
    }
    return smax_tree(q);
}
__device__ __forceinline__ void smax_bwd_finish(const PropSeg &sg, uint32_t lane, double D, double scale, double (&yv)[SMAX_PER_LANE], const double (&gv)[SMAX_PER_LANE],
                                                float *out32, double *out64) {
#pragma clang fp contract(off)
#pragma unroll
    for (uint32_t j = 0; j < SMAX_PER_LANE; j++) {
        const double a = gv[j] - D;
        const double b = a * yv[j];
        yv[j] = b * scale;
    }
    smax_store(sg, lane, yv, out32, out64);
}

template <typename TY, typename TG>
__global__ void __launch_bounds__(BLOCK) k_softmax_bwd_short(const PropSeg *segs, uint64_t nseg, const TY *y, const TG *g, double scale, float *out32, double *out64) {
#pragma clang fp contract(off)
    SMAX_WAVE_PROLOGUE
    double yv[SMAX_PER_LANE], gv[SMAX_PER_LANE];
    const double D = smax_bwd_load(sg, lane, y, g, yv, gv);
    smax_bwd_finish(sg, lane, D, scale, yv, gv, out32, out64);
}

template <typename TY, typename TG>
__global__ void __launch_bounds__(BLOCK) k_softmax_bwd_seg_sum(const PropSeg *segs, uint64_t nseg, const TY *y, const TG *g, double *part) {
#pragma clang fp contract(off)
    SMAX_WAVE_PROLOGUE
    double yv[SMAX_PER_LANE], gv[SMAX_PER_LANE];
    const double P = smax_bwd_load(sg, lane, y, g, yv, gv);
    if (lane == 0) part[u] = P;
}

template <typename TY, typename TG>
__global__ void __launch_bounds__(BLOCK) k_softmax_bwd_div(const PropSeg *segs, uint64_t nseg, const TY *y, const TG *g, double scale, const double *part,
                                                           float *out32, double *out64) {
#pragma clang fp contract(off)
    SMAX_WAVE_PROLOGUE
    double yv[SMAX_PER_LANE], gv[SMAX_PER_LANE];
    (void)smax_bwd_load(sg, lane, y, g, yv, gv);
    smax_bwd_finish(sg, lane, smax_row_sum(sg, part), scale, yv, gv, out32, out64);
}
#undef SMAX_WAVE_PROLOGUE

#if FORA_TEST_PATHS
// exp_def on the device, one point per thread (fora_hip_test_exp, libfora_hip_test.so only)
__global__ void __launch_bounds__(BLOCK) k_softmax_exp(const double *t, uint64_t n, double *out) {
#pragma clang fp contract(off)
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = exp_def(t[i]);
}
#endif

} // namespace fora
