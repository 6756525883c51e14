// LPIPS v0.1 with net='vgg' for the frame-lpips figure of evaluate.py (utils/evaluation/eval_utils.py:368-386 FrameLPIPS: lpips.LPIPS(net='vgg') on the
// frames in 0..255).  The twelve 64-multiple convolutions of torchvision's VGG-16 `features` run on tcl_conv3x3_f16 (bias + ReLU epilogue); this file
// holds the rest of lpips/lpips.py LPIPS.forward and pretrained_networks.py vgg16.
//
// k_lpips_stem (8 lanes per pixel, 8 output channels each): ScalingLayer + features.0 + ReLU from the uint8 frame.  The scaling layer is affine per
//   channel, so its 1 / scale (and the engine's power-of-two input scale) is folded into the 64 x 27 weights on the host and the kernel forms
//   v = x - shift for the pixels inside the frame and 0 outside: Conv2d's zero padding is of the SCALED image, where an outside pixel is 0, not of the
//   uint8 one, where a 0 would scale to -shift / scale.  The weights sit in LDS transposed to [27][64] (the 8 lanes of a pixel read 8 x 32 contiguous
//   bytes, the pixels of a wave the same ones: broadcast), the sums are f32 and the result is rounded once to f16.  No f32 image is written.
// k_maxpool2: MaxPool2d(2, 2), floor mode, 16 bytes of channels per lane.  Of equal values (-0.0 / +0.0) the first in window order wins and a NaN
//   wins over everything, as in torch's max_pool2d.
// k_lpips_head (64 pixels per block, a wave takes 8 at a time, 8 lanes per pixel striding over the channels in 16-byte pieces): normalize_tensor
//   of both feature maps, the squared difference, the `lin` 1x1 convolution and the spatial sum of lpips.py:112-123.  The two channel sums (the
//   norms, then the weighted squared difference) are butterflies over the 8 lanes of a pixel, so every lane holds the same bits; the features are
//   read a second time (from cache) for the difference once the norms are known.  Products are not contracted: for equal inputs n0 - n1 is exactly 0.
//   A block writes its partial sum and the number of non-finite features it saw; nothing is accumulated with atomics.
// k_lpips_finish (one wave per pair): the partials of each tap summed in index order in f64, divided by the tap's pixel count, the taps added in
//   order: spatial_average and the sum over the layers (lpips.py:119-128).  The same input gives the same bits.
#include "common.h"
#include "../../include/tclight_hip.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int STEM_CO = 64, STEM_K = 27;
constexpr int HEAD_PIX = 64;            // pixels per block of the head: 4 waves x 8 pixels x 2 rounds
constexpr int MAX_TAPS = 8;

struct Part { float sum; unsigned bad; };
struct Taps { int n; int P[MAX_TAPS]; int nblk[MAX_TAPS]; };

// ------------------------------------------------------------------------------------------ stem
__global__ __launch_bounds__(256) void k_lpips_stem(const uint8_t* __restrict__ img, const float* __restrict__ w, const float* __restrict__ bias,
                                                    float sh0, float sh1, float sh2, _Float16* __restrict__ y, int H, int W, long npix) {
    __shared__ __align__(16) float ws[STEM_K][STEM_CO];
    __shared__ __align__(16) float bs[STEM_CO];
    const int tid = threadIdx.x;
    for (int i = tid; i < STEM_K * STEM_CO; i += 256) ws[i >> 6][i & 63] = w[(i & 63) * STEM_K + (i >> 6)];
    if (tid < STEM_CO) bs[tid] = bias[tid];
    __syncthreads();
    const int g = tid & 7;
    const float shift[3] = {sh0, sh1, sh2};
    for (long p = (long)blockIdx.x * 32 + (tid >> 3); p < npix; p += (long)gridDim.x * 32) {
        const int x = (int)(p % W);
        const long r = p / W;
        const int yy = (int)(r % H);
        const long b = r / H;
        float acc[8];
        const f4 b0 = *(const f4*)&bs[8 * g], b1 = *(const f4*)&bs[8 * g + 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[j] = b0[j]; acc[4 + j] = b1[j]; }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = yy + ky - 1, ix = x + kx - 1;
                const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
                const uint8_t* s = img + ((b * H + (in ? iy : yy)) * W + (in ? ix : x)) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v = in ? (float)s[c] - shift[c] : 0.f;
                    const float* wr = &ws[(ky * 3 + kx) * 3 + c][8 * g];
                    const f4 w0 = *(const f4*)wr, w1 = *(const f4*)(wr + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { acc[j] = fmaf(v, w0[j], acc[j]); acc[4 + j] = fmaf(v, w1[j], acc[4 + j]); }
                }
            }
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (_Float16)fmaxf(acc[j], 0.f);
        *(h8*)(y + p * STEM_CO + 8 * g) = o;
    }
}

// ------------------------------------------------------------------------------------------ pool
__device__ __forceinline__ h8 pick_max(h8 m, const h8 v) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (v[j] > m[j] || v[j] != v[j]) m[j] = v[j];
    return m;
}

__global__ __launch_bounds__(256) void k_maxpool2(const _Float16* __restrict__ x, _Float16* __restrict__ y, int H, int W, int C, int Ho, int Wo, long n) {
    const int C8 = C / 8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int ch = (int)(i % C8);
        long q = i / C8;
        const int ox = (int)(q % Wo);
        q /= Wo;
        const int oy = (int)(q % Ho);
        const long b = q / Ho;
        const _Float16* s = x + ((b * H + 2 * oy) * W + 2 * ox) * C + ch * 8;
        h8 m = *(const h8*)s;
        m = pick_max(m, *(const h8*)(s + C));
        m = pick_max(m, *(const h8*)(s + (long)W * C));
        m = pick_max(m, *(const h8*)(s + (long)W * C + C));
        *(h8*)(y + i * 8) = m;
    }
}

// ------------------------------------------------------------------------------------------ head
__device__ __forceinline__ float group8_sum(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_lpips_head(const _Float16* __restrict__ f, const float* __restrict__ w, Part* __restrict__ part, int B, int P, int C,
                                                    float eps) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    __shared__ unsigned redb[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, sub = lane & 7, grp = lane >> 3;
    const int b = blockIdx.y, C8 = C / 8;
    const _Float16* f0 = f + (long)b * P * C;
    const _Float16* f1 = f + (long)(B + b) * P * C;
    float acc = 0.f;
    unsigned bad = 0;
    for (int it = 0; it < HEAD_PIX / 32; ++it) {
        const long p = (long)blockIdx.x * HEAD_PIX + it * 32 + wv * 8 + grp;
        const bool live = p < P;                          // a pixel past the end reads the last one and adds nothing: every lane takes part in the shuffles
        const _Float16* a = f0 + (live ? p : (long)P - 1) * C;
        const _Float16* c = f1 + (live ? p : (long)P - 1) * C;
        float s0 = 0.f, s1 = 0.f;
        unsigned nb = 0;
        for (int ch = sub; ch < C8; ch += 8) {
            const h8 va = *(const h8*)(a + ch * 8), vc = *(const h8*)(c + ch * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x0 = (float)va[j], x1 = (float)vc[j];
                s0 += x0 * x0;
                s1 += x1 * x1;
                nb += (isfinite(x0) ? 0u : 1u) + (isfinite(x1) ? 0u : 1u);
            }
        }
        s0 = group8_sum(s0);
        s1 = group8_sum(s1);
        const float r0 = 1.f / (sqrtf(s0) + eps), r1 = 1.f / (sqrtf(s1) + eps);
        float d = 0.f;
        for (int ch = sub; ch < C8; ch += 8) {
            const h8 va = *(const h8*)(a + ch * 8), vc = *(const h8*)(c + ch * 8);
            const f4 w0 = *(const f4*)(w + ch * 8), w1 = *(const f4*)(w + ch * 8 + 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float n0 = (float)va[j] * r0, n1 = (float)vc[j] * r1;
                const float t = n0 - n1;
                d += (j < 4 ? w0[j & 3] : w1[j & 3]) * (t * t);
            }
        }
        if (live) { acc += d; bad += nb; }
    }
    acc = wave_sum(acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if (lane == 0) { red[wv] = acc; redb[wv] = bad; }
    __syncthreads();
    if (tid == 0) {
        Part o;
        o.sum = ((red[0] + red[1]) + red[2]) + red[3];
        o.bad = redb[0] + redb[1] + redb[2] + redb[3];
        part[(long)b * gridDim.x + blockIdx.x] = o;
    }
}

__global__ __launch_bounds__(64) void k_lpips_finish(const Part* __restrict__ part, const Taps t, int B, float* __restrict__ out, int* __restrict__ nonfinite) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double total = 0.0;
    long off = 0;
    for (int k = 0; k < t.n; ++k) {
        const int nb = t.nblk[k];
        const Part* pk = part + off + (long)b * nb;
        double s = 0.0;
        for (int i = lane; i < nb; i += 64) s += (double)pk[i].sum;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        total += s / (double)t.P[k];
        if (b == 0) {
            unsigned long long cnt = 0;
            for (long i = lane; i < (long)B * nb; i += 64) cnt += part[off + i].bad;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
            if (lane == 0) nonfinite[k] = cnt > 0x7fffffffULL ? 0x7fffffff : (int)cnt;
        }
        off += (long)B * nb;
    }
    if (lane == 0) out[b] = (float)total;
}

// the taps' pixel counts -> block counts; false when the list cannot be served
bool make_taps(Taps& t, int B, const int* h_P, int ntaps) {
    if (!(h_P && ntaps >= 1 && ntaps <= MAX_TAPS && B >= 1 && B <= 65535)) return false;
    t.n = ntaps;
    for (int k = 0; k < ntaps; ++k) {
        if (h_P[k] < 1) return false;
        t.P[k] = h_P[k];
        t.nblk[k] = cdiv(h_P[k], HEAD_PIX);
    }
    return true;
}

}  // namespace

extern "C" {

int tcl_lpips_stem_f16(const void* img, const float* w, const float* bias, float shift_r, float shift_g, float shift_b, void* y, int B, int H, int W,
                       hipStream_t st) {
    TCL_CHECK_ARG(img && w && bias && y && B >= 1 && H >= 1 && W >= 1 && (long)B * H * W < (1L << 40));
    const long npix = (long)B * H * W;
    hipLaunchKernelGGL(k_lpips_stem, dim3(stream_grid(npix, 32)), dim3(256), 0, st, (const uint8_t*)img, w, bias, shift_r, shift_g, shift_b, (_Float16*)y, H,
                       W, npix);
    TCL_LAUNCH_RET();
}

int tcl_maxpool2_f16(const void* x, void* y, int B, int H, int W, int C, hipStream_t st) {
    TCL_CHECK_ARG(x && y && B >= 1 && H >= 2 && W >= 2 && C >= 64 && C % 64 == 0);       // H or W of 1: the pooled size would be 0
    const int Ho = H / 2, Wo = W / 2;
    const long n = (long)B * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(k_maxpool2, dim3(stream_grid(n)), dim3(256), 0, st, (const _Float16*)x, (_Float16*)y, H, W, C, Ho, Wo, n);
    TCL_LAUNCH_RET();
}

size_t tcl_lpips_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long)H * W >= (1L << 31)) return 0;
    size_t blocks = 0;
    for (int k = 0; k < 5; ++k) {
        if (H < 1 || W < 1) return 0;                                                    // a pooled size of 0: not a size LPIPS-VGG serves
        blocks += (size_t)cdiv((long)H * W, HEAD_PIX);
        H /= 2; W /= 2;
    }
    return blocks * (size_t)B * sizeof(Part);
}

int tcl_lpips_head(const void* f, const float* w, int B, const int* h_P, int ntaps, int tap, int C, float eps, void* ws, hipStream_t st) {
    Taps t;
    TCL_CHECK_ARG(f && w && ws && make_taps(t, B, h_P, ntaps) && tap >= 0 && tap < ntaps && C >= 64 && C % 64 == 0);
    long off = 0;
    for (int k = 0; k < tap; ++k) off += (long)B * t.nblk[k];
    hipLaunchKernelGGL(k_lpips_head, dim3(t.nblk[tap], B), dim3(256), 0, st, (const _Float16*)f, w, (Part*)ws + off, B, t.P[tap], C, eps);
    TCL_LAUNCH_RET();
}

int tcl_lpips_finish(const void* ws, int B, const int* h_P, int ntaps, float* out, int* nonfinite, hipStream_t st) {
    Taps t;
    TCL_CHECK_ARG(ws && out && nonfinite && make_taps(t, B, h_P, ntaps));
    hipLaunchKernelGGL(k_lpips_finish, dim3(B), dim3(64), 0, st, (const Part*)ws, t, B, out, nonfinite);
    TCL_LAUNCH_RET();
}

}  // extern "C"
