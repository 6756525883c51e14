// light-follow (evaluate.py --light): the ten weighted sums per frame from which the host fits  log-luminance ratio ~ a + gx*u + gy*v  of a relit
// clip E against its source S, gfx950.  The metric is this project's own (the reference has none); its definition is restated in the header.
//
// HBM-bound by design: 6 bytes read per pixel (three u8 planes of E, three of S), one pass, every frame in one launch, then a finish launch.
//
// Who sums what, in which order (the tests hold the kernel to this; nothing here depends on anything but N, H, W):
//   * a frame's H*W pixels are cut into spans of LF_SPAN = LF_ITERS * 256 * 16 = 16384 consecutive pixels, one block of 256 threads per span;
//   * in iteration j < LF_ITERS thread t owns the 16 consecutive pixels from  span*LF_SPAN + j*4096 + t*16 ; it adds the ten terms of its
//     LF_ITERS * 16 = 64 pixels to ten f32 accumulators in pixel order (pixels past the frame's end add nothing);
//   * the accumulators are widened to f64; a wave adds its 64 lanes by a xor butterfly (offsets 32, 16, 8, 4, 2, 1), lane 0 holds the sum;
//   * thread k < 10 adds the four waves' sums of term k in wave order and stores the block's partial to ws[(frame*nb + span)*10 + k];
//   * the finish kernel adds a frame's nb partials in span order.
// No atomics, so two runs give the same bits.  The 16 B path (H*W % 16 == 0, both bases 16 B aligned) and the byte path load the same values into
// the same registers and share everything after the load.
#include "common.h"
#include "../../include/tclight_hip.h"

#define LF_ITERS 4
#define LF_CHUNK 16
#define LF_SPAN (LF_ITERS * 256 * LF_CHUNK)
#define LF_TERMS 10

// x / 255 correctly rounded (what IEEE division gives) for the values the luma takes: q0 = fl(x * fl(1/255)), the exact remainder by one fma,
// one fma to correct (Markstein's sequence for a correctly rounded constant reciprocal).  Equal to the division for every one of the 2^24 (R, G, B)
// triples, checked exhaustively on the host when this was written; the tests hold Sum w, which the result decides, to exact equality.
__device__ __forceinline__ float div255(float x) {
    const float k = 1.f / 255.f;
    const float q0 = x * k;
    const float r = __builtin_fmaf(-q0, 255.f, x);
    return __builtin_fmaf(r, k, q0);
}

// Y = ((0.299 R + 0.587 G) + 0.114 B) / 255 in f32, every product and sum rounded on its own.
__device__ __forceinline__ float luma(unsigned r, unsigned g, unsigned b) {
#pragma clang fp contract(off)
    const float pr = 0.299f * (float)r, pg = 0.587f * (float)g, pb = 0.114f * (float)b;
    const float s = (pr + pg) + pb;
    return div255(s);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// E, S [N,3,hw] u8 -> ws [N,nb,10] f64.  grid (nb, N), 256 threads.
template <bool VEC>
__global__ __launch_bounds__(256) void k_light_fit(const uint8_t* __restrict__ E, const uint8_t* __restrict__ S, int H, int W, int nb,
                                                   double* __restrict__ ws) {
#pragma clang fp contract(off)
    const long hw = (long)H * W;
    const long f = blockIdx.y;
    const uint8_t* pe = E + f * 3 * hw;
    const uint8_t* ps = S + f * 3 * hw;
    const float inv_w = 1.f / (float)W, inv_h = 1.f / (float)H;
    const float lo = 2.f / 255.f, hi = 253.f / 255.f, c = 1.f / 255.f;
    float acc[LF_TERMS];
#pragma unroll
    for (int k = 0; k < LF_TERMS; ++k) acc[k] = 0.f;

#pragma unroll
    for (int j = 0; j < LF_ITERS; ++j) {
        const long p0 = (long)blockIdx.x * LF_SPAN + (long)j * (256 * LF_CHUNK) + (long)threadIdx.x * LF_CHUNK;
        if (p0 >= hw) continue;
        // the six planes' 16 bytes, as four dwords each; VEC: hw % 16 == 0, so p0 + 16 <= hw
        unsigned q[6][4];
        if constexpr (VEC) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                const uint4 a = *(const uint4*)(pe + pl * hw + p0);
                const uint4 b = *(const uint4*)(ps + pl * hw + p0);
                q[pl][0] = a.x; q[pl][1] = a.y; q[pl][2] = a.z; q[pl][3] = a.w;
                q[3 + pl][0] = b.x; q[3 + pl][1] = b.y; q[3 + pl][2] = b.z; q[3 + pl][3] = b.w;
            }
        } else {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    unsigned a = 0, b = 0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const long p = p0 + d * 4 + i;
                        if (p < hw) {
                            a |= (unsigned)pe[pl * hw + p] << (8 * i);
                            b |= (unsigned)ps[pl * hw + p] << (8 * i);
                        }
                    }
                    q[pl][d] = a; q[3 + pl][d] = b;
                }
        }
        int y = (int)(p0 / W), x = (int)(p0 - (long)y * W);
        const int n = hw - p0 < LF_CHUNK ? (int)(hw - p0) : LF_CHUNK;
#pragma unroll
        for (int i = 0; i < LF_CHUNK; ++i) {
            const int d = i >> 2, sh = 8 * (i & 3);
            const float ye = luma((q[0][d] >> sh) & 255u, (q[1][d] >> sh) & 255u, (q[2][d] >> sh) & 255u);
            const float ys = luma((q[3][d] >> sh) & 255u, (q[4][d] >> sh) & 255u, (q[5][d] >> sh) & 255u);
            const bool in = i < n && ye >= lo && ye <= hi && ys >= lo && ys <= hi;
            const float w = in ? 1.f : 0.f;
            const float a = ye + c, b = ys + c;
            const float ratio = a / b;
            const float r = w * logf(ratio);                       // a, b > 0 and finite: the logarithm is finite, w = 0 clears it
            const float u = w * ((float)(x - (W - 1 - x)) * inv_w);   // (2x + 1 - W) / W = (2x + 1)/W - 1
            const float v = w * ((float)(y - (H - 1 - y)) * inv_h);
            acc[0] += w;
            acc[1] += u;
            acc[2] += v;
            acc[3] += u * u;
            acc[4] += u * v;
            acc[5] += v * v;
            acc[6] += r;
            acc[7] += r * u;
            acc[8] += r * v;
            acc[9] += r * r;
            if (++x == W) { x = 0; ++y; }
        }
    }

    __shared__ double red[4][LF_TERMS];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < LF_TERMS; ++k) {
        const double s = wave_sum_f64((double)acc[k]);
        if (lane == 0) red[wid][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < LF_TERMS) {
        const int k = threadIdx.x;
        const double s = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
        ws[(f * nb + blockIdx.x) * LF_TERMS + k] = s;
    }
}

// ws [N,nb,10] -> sums [N,10]: one thread per (frame, term), the partials in span order.
__global__ __launch_bounds__(64) void k_light_fit_finish(const double* __restrict__ ws, int N, int nb, double* __restrict__ sums) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N * LF_TERMS) return;
    const int f = g / LF_TERMS, k = g - f * LF_TERMS;
    const double* p = ws + (long)f * nb * LF_TERMS + k;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += p[(long)b * LF_TERMS];
    sums[g] = s;
}

static bool light_fit_shape_ok(int N, int H, int W) { return N >= 1 && N <= 65535 && H > 0 && W > 0 && (long)H * W < (1L << 31); }
static int light_fit_blocks(int H, int W) { return (int)(((long)H * W + LF_SPAN - 1) / LF_SPAN); }

extern "C" {

size_t tcl_light_fit_workspace_bytes(int N, int H, int W) {
    if (!light_fit_shape_ok(N, H, W)) return 0;
    return (size_t)N * light_fit_blocks(H, W) * LF_TERMS * sizeof(double);
}

int tcl_light_fit_u8(const void* E, const void* S, int N, int H, int W, double* sums, void* ws, hipStream_t st) {
    TCL_CHECK_ARG(E && S && sums && ws && light_fit_shape_ok(N, H, W));
    TCL_CHECK_ARG((((uintptr_t)sums | (uintptr_t)ws) & 7) == 0);
    const long hw = (long)H * W;
    const int nb = light_fit_blocks(H, W);
    const bool vec = hw % 16 == 0 && (((uintptr_t)E | (uintptr_t)S) & 15) == 0;
    auto k = vec ? k_light_fit<true> : k_light_fit<false>;
    hipLaunchKernelGGL(k, dim3(nb, N), dim3(256), 0, st, (const uint8_t*)E, (const uint8_t*)S, H, W, nb, (double*)ws);
    hipLaunchKernelGGL(k_light_fit_finish, dim3(cdiv((long)N * LF_TERMS, 64)), dim3(64), 0, st, (const double*)ws, N, nb, sums);
    TCL_LAUNCH_RET();
}

}  // extern "C"
