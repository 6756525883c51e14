// Shared between gemm.hip and gemm8.hip: implicit-GEMM 3x3 convolution descriptor and the 8-wave kernel entry.
#pragma once
#include <hip/hip_runtime.h>
#include "attn_panels.h"

struct ConvP {
    int conv;            // 0: dense A[M][lda]; 1: implicit 3x3
    int Hin, Win, Cin;   // stored input (before optional upsample)
    int Hup, Wup;        // logical input size seen by the conv (== Hin,Win unless nearest-upsampled)
    int Hout, Wout, stride, pad;
    float sy, sx;        // Hin/Hup, Win/Wup (nearest source scale, PyTorch 'nearest' convention)
};

// QKV projection written straight into the flash kernel's panels (round 5; csrc/attn.hip documents the layouts, attn_panels.h defines them): Qp [ne, H, Tqp, DP] pre-scaled,
// Kp [ne, H, Tkp, KS] (+ ones column `one_col` when >= 0), Vt [ne, H, Tkp / 64, vtile halves]: DPV rows of V_STRIDE halves per 64-key tile, keys permuted
// (bits 2 <-> 3 of the in-tile key index), rows 4..11 (mod 16) skewed by 16 positions when `skew`, row d = ones over the valid keys when DPV > d.
// Everything the epilogue does not write (padding rows / columns, rows d + 1 .. DPV - 1) is expected to be ZERO already.
// aidx (may be null): token t of an entry reads row aidx[t] of that entry's source block (the VidToMe merge map: the merged sequence is never gathered into
// a tensor of its own); a_bs: elements between the entries' source blocks.
struct QkvPanel { _Float16 *qp, *kp, *vt; int T, Tqp, Tkp, H, d, DP, KS, DPV, vtile, one_col, skew; float qscale; const int* aidx; long a_bs; };
int gemm_dma_qkv_panels(const _Float16* A, const _Float16* W, int ne, int K, int lda, int ldw, const QkvPanel& qp, hipStream_t st);

// K order of the implicit 3x3 convolution, shared by every GEMM kernel so that they all accumulate in the same order (results are
// bit-identical across tile configurations).  The weights are stored tap-major ([Cout][9][Cin]); the kernels WALK K channel-slice-major
// when Cin % 64 == 0: the 64-wide step q covers channels (q/9)*64.. of tap q%9, so nine consecutive steps re-touch the same input rows
// (one 128-B line per pixel, L1/L2-resident) instead of striding through all Cin channels of one tap.  k0 is the linear step start
// (a multiple of 32); returns the tap and sets c0 (channel offset); the weight column is tap*Cin + c0.
__device__ __forceinline__ int conv_kmap(int k0, int Cin, int& c0) {
    if ((Cin & 63) == 0) { const int q = k0 >> 6, c64 = q / 9; c0 = c64 * 64 + (k0 & 63); return q - c64 * 9; }
    const int tap = k0 / Cin; c0 = k0 - tap * Cin; return tap;
}

// erf-GELU for epilogues whose input and output are f16: erf by Abramowitz-Stegun 7.1.26 (|error| < 1.5e-7, far below the f16 rounding of the
// result) -- one v_rcp, one v_exp and 9 fma / mul instead of libdevice erff's two-branch evaluation (~28 vector instructions per element;
// the GEGLU epilogue of a K = 320 Linear issues more vector cycles than its ten K steps issue matrix cycles)
__device__ __forceinline__ float gelu_erf(float v) {
    const float x = v * 0.70710678f, ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f); p = fmaf(p, t, -0.284496736f); p = fmaf(p, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(ax * ax * -TCL_LOG2E);
    const float erfa = fmaf(-(p * t), e, 1.f);                     // erf(|x|)
    return 0.5f * v * (1.f + copysignf(erfa, x));
}

// epilogue activations: 1 SiLU, 3 ReLU, 4 GELU (erf); 0, 2 (GEGLU, applied on column pairs by the caller) and 5 (GELU applied AFTER the
// residual add, see post_act) leave v unchanged
__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == 1) return v / (1.f + __expf(-v));
    if (act == 3) return fmaxf(v, 0.f);
    if (act == 4) return gelu_erf(v);
    return v;
}

__device__ __forceinline__ float post_act(float v, int act) { return act == 5 ? gelu_erf(v) : v; }

// One GEMM / implicit-convolution call as every host function of the dispatch sees it: the operands, the problem, the epilogue and the stream.
// The C-ABI entries build it once; launchers read the kernel arguments from it one by one.
struct GemmCall {
    const _Float16 *A, *W, *bias, *resid; _Float16* C;
    int M, N, K, lda, ldw, ldc, ldr, act;
    ConvP cp;
    hipStream_t st;
    bool has_resid() const { return resid != nullptr; }
    // extents of A (dense, or the stored NHWC input of a convolution) and of W in bytes: what 32-bit offsets have to reach
    size_t a_bytes() const { return cp.conv ? (size_t)(M / (cp.Hout * cp.Wout)) * cp.Hin * cp.Win * cp.Cin * 2 : ((size_t)(M - 1) * lda + K) * 2; }
    size_t w_bytes() const { return ((size_t)(N - 1) * ldw + K) * 2; }
};

// 8-wave ping-pong kernels (gemm8.hip), by tile
int gemm8_256x320(const GemmCall& c), gemm8_128x320(const GemmCall& c), gemm8_256x256(const GemmCall& c), gemm8_128x256(const GemmCall& c);
// 8-phase 256-row kernels (gemm8q.hip), by tile; gemm8q_ok: can the tile of width BN (256, 320; 128 = the 512-row tile) take this call?
bool gemm8q_ok(int BN, const GemmCall& c);
int gemm8q_256x256(const GemmCall& c), gemm8q_256x320(const GemmCall& c), gemm8q_512x128(const GemmCall& c);
// strip-resident K = 320 Linear (linstrip.hip); revisits_resid: an in-place residual on a call whose last weight tile is moved back -- not for this
// kernel; gamma / beta: LayerNorm folded into the A load
bool lin_strip_ok(const GemmCall& c), lin_strip_revisits_resid(const GemmCall& c);
int lin_strip_dispatch(const GemmCall& c, const _Float16* gamma = nullptr, const _Float16* beta = nullptr, float eps = 0.f);
