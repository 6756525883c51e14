// RAFT update block and fnet stem (utils/evaluation/core/update.py:33-136, extractor.py:139-172) -- the pieces the MemFlowNet kernels do not cover.
//
// k_sepconv: one half-step of SepConvGRU (update.py:33-56) as implicit GEMMs over NHWC f16 rows with f16 MFMA and f32 accumulation.  The
// convolution is 1x5 (pad (0,2)) or 5x1 (pad (2,0)) over x = [src0 | src1] (128 channels each, src1 may be absent).  K is walked tap-major
// (tap, source, 64-channel slice), the weight is W[N][5 * (C0 + C1)] with column tap * (C0 + C1) + source * C0 + c.  Epilogues:
//   mode 0 (fold)      : out32[m, n] = acc + bias[n]                                        -- the context term conv(inp) + bias, once per pair
//   mode 1 (gate)      : v = acc + pb[m, n]; n < 128: z[m, n] = sigmoid(v) (f32);
//                        n >= 128: rh[m, n - 128] = f16(sigmoid(v) * h[m, n - 128])       -- [z | r] as one N = 256 GEMM, r * h for the q conv
//   mode 2 (candidate) : q = tanh(acc + pb[m, n]); h[m, n] = f16((1 - z) h + z q)          -- in place, blend in f32, one rounding
// Tile 64 rows x 128 columns, 4 waves of 32 x 64 (two mfma_f32_32x32x16_f16 accumulators each), BK = 64 (one tap of one 64-channel slice),
// LDS double-buffered with the next slice held in registers across the MFMAs.
#include "common.h"
#include "../../include/tclight_hip.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));

namespace {

constexpr int BM = 64, BN = 128, BK = 64, LDK = BK + 8;    // +8 halves per LDS row: the 32 rows a fragment read touches fall in different banks

struct SepArgs {
    const _Float16* s0; const _Float16* s1; int C1;           // sources: s0 [M,128], s1 [M,128] (C1 = 0: absent)
    const _Float16* w; const float* bias; const float* pb;    // W [N, 5 (128 + C1)], channel bias (mode 0), per-pixel bias [M, N] (modes 1, 2)
    float* out32; float* z; _Float16* rh; _Float16* h;
    int M, N, H, W, vertical, mode;
};

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + __expf(-v)); }

__global__ __launch_bounds__(256) void k_sepconv(SepArgs a) {
    __shared__ _Float16 sA[2][BM * LDK];
    __shared__ _Float16 sB[2][BN * LDK];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int Ctot = 128 + a.C1, nslice = Ctot / 64, steps = 5 * nslice, K = 5 * Ctot;
    const int HW = a.H * a.W;
    // A staging: 64 rows x 8 chunks of 16 B -> 2 chunks per thread (rows tid / 8 and tid / 8 + 32, chunk tid % 8)
    const int ar = tid >> 3, ac = (tid & 7) * 8;
    int pos[2]; bool rin[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + ar + 32 * i;
        rin[i] = m < a.M;
        const int p = m % HW;
        pos[i] = a.vertical ? p / a.W : p % a.W;                  // coordinate along the tap axis
    }
    const int stride = a.vertical ? a.W : 1, extent = a.vertical ? a.H : a.W;
    // B staging: 128 rows x 8 chunks -> 4 chunks per thread (rows tid / 8 + 32 j)
    h8 ra[2], rb[4];
    auto load = [&](int s) {
        const int tap = s / nslice, sl = s - tap * nslice;
        const _Float16* src = sl < 2 ? a.s0 : a.s1;
        const int c0 = (sl & 1) * 64 + ac, d = tap - 2;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = pos[i] + d;
            if (rin[i] && q >= 0 && q < extent) ra[i] = *(const h8*)(src + (long)(m0 + ar + 32 * i + d * stride) * 128 + c0);
            else ra[i] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
        }
        const int kc = tap * Ctot + sl * 64 + ac;
#pragma unroll
        for (int j = 0; j < 4; ++j) rb[j] = *(const h8*)(a.w + (long)(n0 + ar + 32 * j) * K + kc);
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *(h8*)(&sA[buf][(ar + 32 * i) * LDK + ac]) = ra[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) *(h8*)(&sB[buf][(ar + 32 * j) * LDK + ac]) = rb[j];
    };
    f16v acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int wr = (wv & 1) * 32, wc = (wv >> 1) * 64, fr = lane & 31, fk = (lane >> 5) * 8;
    load(0); store(0);
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int buf = s & 1;
        if (s + 1 < steps) load(s + 1);
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            const h8 fa = *(const h8*)(&sA[buf][(wr + fr) * LDK + ks * 16 + fk]);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const h8 fb = *(const h8*)(&sB[buf][(wc + 32 * t + fr) * LDK + ks * 16 + fk]);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc[t], 0, 0, 0);
            }
        }
        if (s + 1 < steps) store(buf ^ 1);
        __syncthreads();
    }
    // epilogue: lane owns column n = n0 + wc + 32 t + (lane & 31), rows m0 + wr + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = n0 + wc + 32 * t + fr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wr + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m >= a.M) continue;
            float v = acc[t][r];
            if (a.mode == 0) {
                a.out32[(long)m * a.N + n] = v + a.bias[n];
            } else if (a.mode == 1) {
                const float g = sigmoidf_(v + a.pb[(long)m * a.N + n]);
                if (n < 128) a.z[(long)m * 128 + n] = g;
                else a.rh[(long)m * 128 + n - 128] = (_Float16)(g * (float)a.h[(long)m * 128 + n - 128]);
            } else {
                const float q = tanhf(v + a.pb[(long)m * 128 + n]), z = a.z[(long)m * 128 + n];
                const float hv = (float)a.h[(long)m * 128 + n];
                a.h[(long)m * 128 + n] = (_Float16)((1.f - z) * hv + z * q);
            }
        }
    }
}

// convf1 (update.py:69,75): relu(Conv2d(2, 128, 7, padding=3)(coords1 - coords0)), coords0 being the pixel grid (coords_grid, utils.py:83-86) that
// is subtracted here in f32 exactly as the reference subtracts it.  coords1 [B,2,H,W] f32 NCHW -> f16 rows [B*H*W, ldo], channels 0..127.
// VALU: K = 98 is a fraction of one MFMA K-tile.  Wave w of a block owns 32 output channels of the block's 64 pixels; its weight reads are
// wave-uniform (scalar loads).  w_t [98][128] f32, row c * 49 + ky * 7 + kx.
__global__ __launch_bounds__(256) void k_convf1(const float* __restrict__ c1, const float* __restrict__ wt, const float* __restrict__ bias,
                                                _Float16* __restrict__ y, int ldo, int B, int H, int W) {
    const int HW = H * W;
    const long gp = (long)blockIdx.x * 64 + (threadIdx.x & 63);
    const int cg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * 32;
    if (gp >= (long)B * HW) return;
    const int b = (int)(gp / HW), p = (int)(gp - (long)b * HW), py = p / W, px = p - py * W;
    float acc[32];
#pragma unroll
    for (int o = 0; o < 32; ++o) acc[o] = bias[cg + o];
    for (int c = 0; c < 2; ++c) {
        const float* src = c1 + ((long)b * 2 + c) * HW;
        for (int ky = 0; ky < 7; ++ky) {
            const int iy = py - 3 + ky;
            if (iy < 0 || iy >= H) continue;
            for (int kx = 0; kx < 7; ++kx) {
                const int ix = px - 3 + kx;
                if (ix < 0 || ix >= W) continue;
                const float v = src[(long)iy * W + ix] - (float)(c == 0 ? ix : iy);
                const float* wr = wt + (c * 49 + ky * 7 + kx) * 128 + cg;
#pragma unroll
                for (int o = 0; o < 32; ++o) acc[o] = fmaf(v, wr[o], acc[o]);
            }
        }
    }
    _Float16* dst = y + gp * ldo + cg;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        h8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (_Float16)fmaxf(acc[q * 8 + j], 0.f);
        *(h8*)(dst + q * 8) = v;
    }
}

// fnet stem (extractor.py:139,164-166) with the convolution output kept in f32 up to the instance norm: conv7x7 stride 2 pad 3 on [B,3,H,W] f32 NCHW ->
// [B,Ho,Wo,64] f32 NHWC; w_t [147][64] f32, row c * 49 + ky * 7 + kx.
__global__ __launch_bounds__(256) void k_conv7x7s2_f32(const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias,
                                                       float* __restrict__ y, int H, int W, int Ho, int Wo) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x, P = Ho * Wo;
    if (p >= P) return;
    const int oy = p / Wo, ox = p - oy * Wo;
    float acc[64];
#pragma unroll
    for (int o = 0; o < 64; ++o) acc[o] = bias[o];
    for (int c = 0; c < 3; ++c) {
        const float* src = x + ((long)b * 3 + c) * H * W;
        for (int ky = 0; ky < 7; ++ky) {
            const int iy = oy * 2 - 3 + ky;
            if (iy < 0 || iy >= H) continue;
            for (int kx = 0; kx < 7; ++kx) {
                const int ix = ox * 2 - 3 + kx;
                if (ix < 0 || ix >= W) continue;
                const float v = src[(long)iy * W + ix];
                const float* wr = wt + (c * 49 + ky * 7 + kx) * 64;
#pragma unroll
                for (int o = 0; o < 64; ++o) acc[o] = fmaf(v, wr[o], acc[o]);
            }
        }
    }
    float4* dst = (float4*)(y + ((long)b * P + p) * 64);
#pragma unroll
    for (int q = 0; q < 16; ++q) dst[q] = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
}

// InstanceNorm2d(64) + ReLU over f32 NHWC [B,HW,64] -> f16 rows.  Two passes (mean, then the centred sum of squares): with [0, 1] images the
// per-channel spread is ~1 % of the stem's constant part, where E[x^2] - mean^2 would cancel most of the f32 digits.  Deterministic: fixed-order
// per-block partials, reduced in block order.
constexpr int IN_C = 64;
__global__ __launch_bounds__(256) void k_in32_partial(const float* __restrict__ x, const float* __restrict__ mean, int HW, int rpb, float* __restrict__ part) {
    __shared__ float ps[4][IN_C];
    const int b = blockIdx.y, c = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, HW);
    const float mu = mean ? mean[b * IN_C + c] : 0.f;
    float s = 0.f;
    for (int r = r0 + ph; r < r1; r += 4) {
        const float v = x[((long)b * HW + r) * IN_C + c];
        s += mean ? (v - mu) * (v - mu) : v;
    }
    ps[ph][c] = s;
    __syncthreads();
    if (ph == 0) part[((long)b * gridDim.x + blockIdx.x) * IN_C + c] = ((ps[0][c] + ps[1][c]) + ps[2][c]) + ps[3][c];
}
__global__ void k_in32_reduce(const float* __restrict__ part, int nblk, float inv_n, float eps, int final_, float* __restrict__ out) {
    const int b = blockIdx.x, c = threadIdx.x;
    float s = 0.f;
    for (int i = 0; i < nblk; ++i) s += part[((long)b * nblk + i) * IN_C + c];
    out[b * IN_C + c] = final_ ? rsqrtf(s * inv_n + eps) : s * inv_n;
}
__global__ void k_in32_apply(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd, _Float16* __restrict__ y, int B, int HW) {
    const long total = (long)B * HW * (IN_C / 8);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i >> 3; const int ch = (int)(i & 7) * 8, b = (int)(row / HW);
        const float4 u = *(const float4*)(x + row * IN_C + ch), v = *(const float4*)(x + row * IN_C + ch + 4);
        const float e[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (_Float16)fmaxf((e[j] - mean[b * IN_C + ch + j]) * rstd[b * IN_C + ch + j], 0.f);
        *(h8*)(y + row * IN_C + ch) = o;
    }
}

}  // namespace

extern "C" {

int tcl_raft_sepconv_f16(const void* src0, const void* src1, int C1, const void* w, const float* bias, const float* pbias, float* out32, float* z,
                         void* rh, void* h, int B, int H, int W, int N, int vertical, int mode, hipStream_t st) {
    TCL_CHECK_ARG(src0 && w && B > 0 && H > 0 && W > 0 && (C1 == 0 || (C1 == 128 && src1)) && (vertical == 0 || vertical == 1));
    TCL_CHECK_ARG(N % BN == 0 && N > 0);
    if (mode == 0) TCL_CHECK_ARG(bias && out32);
    else if (mode == 1) TCL_CHECK_ARG(N == 256 && pbias && z && rh && h);
    else if (mode == 2) TCL_CHECK_ARG(N == 128 && pbias && z && h);
    else return TCL_EINVAL;
    SepArgs a{(const _Float16*)src0, (const _Float16*)src1, C1, (const _Float16*)w, bias, pbias, out32, z, (_Float16*)rh, (_Float16*)h,
              B * H * W, N, H, W, vertical, mode};
    hipLaunchKernelGGL(k_sepconv, dim3(cdiv((long)a.M, BM), N / BN), dim3(256), 0, st, a);
    TCL_LAUNCH_RET();
}

int tcl_raft_convf1_f16(const float* coords1, const float* w_t, const float* bias, void* y, int ldo, int B, int H, int W, hipStream_t st) {
    TCL_CHECK_ARG(coords1 && w_t && bias && y && ldo >= 128 && ldo % 8 == 0 && B > 0 && H > 0 && W > 0);
    hipLaunchKernelGGL(k_convf1, dim3(cdiv((long)B * H * W, 64)), dim3(256), 0, st, coords1, w_t, bias, (_Float16*)y, ldo, B, H, W);
    TCL_LAUNCH_RET();
}

size_t tcl_stem_instnorm_workspace_bytes(int B, int H, int W) {
    const long P = (long)((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
    return ((size_t)B * P * IN_C + (size_t)B * 256 * IN_C + (size_t)B * IN_C * 2) * 4 + 256;
}

int tcl_conv7x7s2_instnorm_f16(const float* x, const float* w_t, const float* bias, void* y, int B, int H, int W, float eps, void* ws, hipStream_t st) {
    TCL_CHECK_ARG(x && w_t && bias && y && ws && B > 0 && H > 0 && W > 0);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, HW = Ho * Wo;
    float* s32 = (float*)ws; float* part = s32 + (size_t)B * HW * IN_C; float* mean = part + (size_t)B * 256 * IN_C; float* rstd = mean + B * IN_C;
    hipLaunchKernelGGL(k_conv7x7s2_f32, dim3(cdiv(HW, 256), B), dim3(256), 0, st, x, w_t, bias, s32, H, W, Ho, Wo);
    int nblk = cdiv(HW, 256); nblk = nblk > 256 ? 256 : nblk;
    const int rpb = cdiv(HW, nblk); nblk = cdiv(HW, rpb);
    hipLaunchKernelGGL(k_in32_partial, dim3(nblk, B), dim3(256), 0, st, s32, (const float*)nullptr, HW, rpb, part);
    hipLaunchKernelGGL(k_in32_reduce, dim3(B), dim3(IN_C), 0, st, part, nblk, 1.f / (float)HW, eps, 0, mean);
    hipLaunchKernelGGL(k_in32_partial, dim3(nblk, B), dim3(256), 0, st, s32, (const float*)mean, HW, rpb, part);
    hipLaunchKernelGGL(k_in32_reduce, dim3(B), dim3(IN_C), 0, st, part, nblk, 1.f / (float)HW, eps, 1, rstd);
    hipLaunchKernelGGL(k_in32_apply, dim3(stream_grid((long)B * HW * 8, 256, 2)), dim3(256), 0, st, s32, mean, rstd, (_Float16*)y, B, HW);
    TCL_LAUNCH_RET();
}

}  // extern "C"
