// What more than one of the Cholesky sources uses (kernels_chol_step.hip, kernels_chol_dataflow.hip,
// kernels_backsolve.hip): LDS strides, the 8x8 pivot block in registers, the bounded-spin contract and the
// inverse of a diagonal factor.  Device code only.
#pragma once
#include "engine.hpp"

namespace vmm {

constexpr int kLd = 65;   // LDS row stride of the 64x64 diagonal block (odd -> conflict-free columns)
constexpr int kLdT = 66;  // row stride of its transposed copy (even -> 16-B aligned 4-column groups)

typedef double double4_t __attribute__((ext_vector_type(4)));

// 1/sqrt(v) on the 64-deep dependent pivot chain: hardware v_rsq_f64 seed plus one third-order
// correction (the same polynomial the device math library uses), branch-free.  ~1 ulp.
// The validity test is NOT on the chain: a non-positive or non-finite pivot yields NaN (rsq of a negative
// number, 0 * inf in the correction), which poisons this factorisation only -- the caller raises lin_fail
// from `ok`, the LM loop rejects the step and rebuilds the reduced system from scratch.
__device__ __forceinline__ double safe_rsqrt(double v, bool& ok)
{
    ok = ok && (v > 0.0) && isfinite(v);
    const double y0 = __builtin_amdgcn_rsq(v);
    const double e = fma(-v * y0, y0, 1.0);
    return fma(y0 * e, fma(e, 0.375, 0.5), y0);
}

// block structure of a tree-ordered factor (DfArgs::nz): bit k of block row i
__device__ __forceinline__ bool nz_bit(const unsigned long long* nz, const int i, const int k)
{
    return (nz[kDfMaskWords * i + (k >> 6)] >> (k & 63)) & 1ull;
}

constexpr int kPs = 9;   // LDS row stride (doubles) of the 64x8 panel buffers: conflict-free rows
constexpr int kPw = 8;   // columns per round

__device__ __forceinline__ constexpr int tri8(int r, int c) { return r * (r + 1) / 2 + c; }

struct Piv8 {
    double l[36];     // lower triangle of the 8x8 factor, packed row-major (diagonal included)
    double inv[8];    // reciprocals of its diagonal
    bool ok;
};

// Cholesky of the symmetric 8x8 block at D (LDS, row stride kPs, lower triangle), in registers.
// Right-looking: as soon as column j is scaled, its outer product is subtracted from the columns to its right, so
// the NEXT pivot depends on one multiply and one fused multiply-add behind the reciprocal square root instead of
// on a j-deep chain of dependent FMAs (the left-looking form cost ~143 cycles per pivot, this one ~100); the other
// updates are independent and fill the issue slots the chain leaves free.
__device__ __forceinline__ void chol8(const double* __restrict__ D, Piv8& p)
{
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c)
            p.l[tri8(r, c)] = D[r * kPs + c];
    p.ok = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double t = p.l[tri8(j, j)];
        bool okj = true;
        const double inv = safe_rsqrt(t, okj);
        p.ok = p.ok && okj;
        p.inv[j] = inv;
        p.l[tri8(j, j)] = t * inv;
#pragma unroll
        for (int i = j + 1; i < 8; ++i)
            p.l[tri8(i, j)] *= inv;
        // the next pivot's diagonal first
#pragma unroll
        for (int c = j + 1; c < 8; ++c)
#pragma unroll
            for (int i = c; i < 8; ++i)
                p.l[tri8(i, c)] = fma(-p.l[tri8(i, j)], p.l[tri8(c, j)], p.l[tri8(i, c)]);
    }
}

// x <- x L8^{-T} (a row of eight columns scaled by the pivot block's factor), right-looking for the same reason:
// every step is one multiply behind the previous step's update instead of a q-deep chain.
__device__ __forceinline__ void scale8(double (&x)[8], const Piv8& p)
{
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        x[q] *= p.inv[q];
#pragma unroll
        for (int c = q + 1; c < 8; ++c)
            x[c] = fma(-x[q], p.l[tri8(c, q)], x[c]);
    }
}

constexpr unsigned kSpinLimit = 1u << 22;   // polls of a chain hand-off (the dataflow kernels: kDfSpinDefault)

// one thread: this pass gave up waiting in kernel `bit` (1 dataflow factorisation, 2 back-substitution chain)
__device__ __forceinline__ void raise_sync_timeout(LmCtl* ctl, int bit)
{
    atomicOr(&ctl->sync_timeout, bit);
    atomicExch(&ctl->done, 2);
}

// Explicit inverse of one 64x64 lower-triangular diagonal factor (for the chained back-substitution,
// which then needs a 64x64 GEMV per block instead of 16 dependent 4x4 solves).  One wave, thread c
// solves L x = e_c; entries above row c are zero, so all lanes run the same 2016 multiply-adds.
// Runs as one extra workgroup of a later launch, beside the latency-bound panel: free.
// L (row stride kLd, upper part zero) and di (reciprocal diagonal) already in LDS; wave 0 computes.
__device__ __forceinline__ void chol_inverse_lds(const double* L, const double* di, double* __restrict__ Linvk)
{
    const int tid = threadIdx.x;
    if (tid >= 64)
        return;
    const int c = tid;
    double x[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
        for (int m = 0; m + 3 < i; m += 4) {
            s0 += L[i * kLd + m] * x[m];
            s1 += L[i * kLd + m + 1] * x[m + 1];
            s2 += L[i * kLd + m + 2] * x[m + 2];
            s3 += L[i * kLd + m + 3] * x[m + 3];
        }
#pragma unroll
        for (int m = (i / 4) * 4; m < i; ++m)
            s0 += L[i * kLd + m] * x[m];
        const double s = (s0 + s1) + (s2 + s3);
        x[i] = (i == c) ? di[i] : ((i < c) ? 0.0 : -s * di[i]);
        Linvk[i * 64 + c] = x[i];
    }
}

__device__ __forceinline__ void chol_inverse_wg(const double* __restrict__ Ldk, const double* __restrict__ dinvk,
                                                double* __restrict__ Linvk, double* smem)
{
    double* L = smem;
    double* di = smem + 64 * kLd;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < 64 * 64; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        L[r * kLd + c] = (c <= r) ? Ldk[idx] : 0.0;
    }
    if (tid < 64)
        di[tid] = dinvk[tid];
    __syncthreads();
    chol_inverse_lds(L, di, Linvk);
}

} // namespace vmm
