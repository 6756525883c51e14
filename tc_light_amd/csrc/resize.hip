// The highres pass (IC-Light's process(), gradio_demo_iclight.py:301-334: highres_scale, highres_denoise), gfx950: what lies between the first pass's
// VAE decode and the second pass's VAE encode.
//   * k_frames_to_u8: decoded frames [N,3,H,W] f32 -> [N,H,W,3] u8, u = trunc(clamp(fl32(255*p), 0, 255)), no fma contraction;
//   * k_resize_lanczos: PIL's Image.resize((Wo, Ho), Image.LANCZOS) on [N,H,W,3] u8, bit for bit;
//   * k_u8_to_frames: [N,H,W,3] u8 -> [N,3,H,W] f32 = u / denom (one IEEE division; denom 254 is the demo's u/127 - 1 in VAEEngine.encode's convention).
//
// PIL's resampler (Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc) is integer arithmetic once its
// coefficients exist: per output index the Lanczos-3 weights over a support widened by the down-scale factor are computed in f64, normalised and rounded
// half away from zero to 22-bit fixed point; an accumulator starts at 1 << 21, is shifted right by 22 and clipped to u8; the horizontal pass is clipped
// to u8 before the vertical pass reads it; an axis whose size does not change is not resampled.  The weights contain sin(), and one flipped coefficient
// breaks bit-identity, so the tables are made on the HOST with the C library (tcl_resize_lanczos_table) and uploaded by the caller; the kernel only
// does the integer part.
//
// k_resize_lanczos<KX, KY>: one block (256 threads) per RT_X x RT_Y tile of one output frame.  The tile's coefficient rows and bounds go to LDS, the
// input rows its vertical taps touch are resampled horizontally into LDS (u8, RT_X * 3 bytes per row), and the vertical pass reads them from there.  In
// the horizontal pass a lane owns one byte of a row and loads its K source bytes before the first multiply; in the vertical pass it owns 4 consecutive
// bytes, loads K LDS dwords and stores one dword.  K is a template parameter and the tap loops are unrolled; taps past a window's count have
// coefficient 0 and a clamped address.  KX / KY: 0 = that axis is not resampled, 7 = an up-scale (ksize 7), 13 = a down-scale up to 2 (ksize 9, 11 or 13).
#include "common.h"
#include "../../include/tclight_hip.h"
#include <math.h>

namespace {

constexpr int PBITS = 32 - 8 - 2;       // PIL's PRECISION_BITS
constexpr int RT_X = 32, RT_Y = 64;     // output tile
constexpr int ROWB = RT_X * 3;          // bytes of a tile row
constexpr int KMAX = 13;                // ksize at in / out = 2

inline bool axis_ok(int in, int out) { return in > 0 && out > 0 && (long)in * 4 >= out && in <= 2L * out; }
inline double axis_support(int in, int out) {
    const double scale = (double)in / (double)out;
    return 3.0 * (scale < 1.0 ? 1.0 : scale);
}
inline int axis_ksize(int in, int out) { return (int)ceil(axis_support(in, out)) * 2 + 1; }

inline double lanczos3(double x) {      // Resample.c: lanczos_filter over sinc_filter
#pragma clang fp contract(off)
    if (-3.0 <= x && x < 3.0) {
        const double y = x / 3, a = x * M_PI, b = y * M_PI;      // sinc_filter(x) * sinc_filter(x / 3)
        const double sa = x == 0.0 ? 1.0 : sin(a) / a, sb = y == 0.0 ? 1.0 : sin(b) / b;
        return sa * sb;
    }
    return 0.0;
}

__device__ __forceinline__ int clip8(int v) { return min(max(v >> PBITS, 0), 255); }
__device__ __forceinline__ unsigned pack4(const int v[4]) { return (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24); }

// tx / ty: [out][2] bounds (first input index, tap count) followed by [out][ksize] taps, as tcl_resize_lanczos_table writes them
template <int KX, int KY>
__global__ __launch_bounds__(256) void k_resize_lanczos(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int Ho, int Wo,
                                                        const int* __restrict__ tx, const int* __restrict__ ty, int ksx, int ksy, int max_rows, int vec) {
    extern __shared__ __align__(16) unsigned char smem[];
    int* kx = (int*)smem;                            // [RT_X][KMAX]
    int* ky = kx + RT_X * KMAX;                      // [RT_Y][KMAX]
    int* bx = ky + RT_Y * KMAX;                      // [RT_X]: first input column of every output column (taps past a window's count are 0)
    int* by = bx + RT_X;                             // [RT_Y][2]: first input row, tap count
    uint8_t* hrow = (uint8_t*)(by + RT_Y * 2);       // [max_rows][ROWB]: the horizontally resampled input rows of the tile
    const int tid = threadIdx.x, n = blockIdx.z;
    const int ox0 = blockIdx.x * RT_X, oy0 = blockIdx.y * RT_Y;
    // output indices past the image are clamped (their results are never stored); bounds are clamped to the input whatever the table holds
    if (KX) {
        for (int i = tid; i < RT_X * KMAX; i += 256) {
            const int col = i / KMAX, t = i - col * KMAX, o = min(ox0 + col, Wo - 1);
            kx[i] = t < ksx ? tx[2 * Wo + o * ksx + t] : 0;
        }
        if (tid < RT_X) {
            const int o = min(ox0 + tid, Wo - 1);
            bx[tid] = min(max(tx[2 * o], 0), W - 1);
        }
    }
    if (KY) {
        for (int i = tid; i < RT_Y * KMAX; i += 256) {
            const int row = i / KMAX, t = i - row * KMAX, o = min(oy0 + row, Ho - 1);
            ky[i] = t < ksy ? ty[2 * Ho + o * ksy + t] : 0;
        }
        if (tid >= 64 && tid < 64 + RT_Y) {
            const int r = tid - 64, o = min(oy0 + r, Ho - 1);
            const int lo = min(max(ty[2 * o], 0), H - 1);
            by[2 * r] = lo; by[2 * r + 1] = min(max(ty[2 * o + 1], 0), min(ksy, H - lo));
        }
    }
    __syncthreads();
    const int y0 = KY ? by[0] : oy0;
    const int rows = KY ? max(min(by[2 * (RT_Y - 1)] + by[2 * (RT_Y - 1) + 1] - y0, max_rows), 1) : RT_Y;
    const uint8_t* fr = src + (long)n * H * W * 3;
    for (int item = tid; item < rows * ROWB; item += 256) {
        const int r = item / ROWB, e = item - r * ROWB, col = e / 3, c = e - col * 3;
        const uint8_t* line = fr + (long)min(y0 + r, H - 1) * W * 3 + c;
        int v;
        if (KX) {
            const int lo = bx[col];
            const int* k = kx + col * KMAX;
            int px[KX ? KX : 1];             // one register per source byte: all KX loads are in flight before the first multiply
#pragma unroll
            for (int t = 0; t < KX; ++t) px[t] = line[(long)min(lo + t, W - 1) * 3];
            int ss = 1 << (PBITS - 1);
#pragma unroll
            for (int t = 0; t < KX; ++t) ss += px[t] * k[t];
            v = clip8(ss);
        } else {
            v = line[(long)min(ox0 + col, W - 1) * 3];
        }
        hrow[item] = (uint8_t)v;
    }
    __syncthreads();
    uint8_t* out = dst + (long)n * Ho * Wo * 3;
    for (int item = tid; item < RT_Y * (ROWB / 4); item += 256) {
        const int row = item / (ROWB / 4), g = item - row * (ROWB / 4);
        const int oy = oy0 + row;
        if (oy >= Ho) break;                         // rows are visited in order: nothing further down is inside either
        const int e0 = 4 * g, valid = min(Wo - ox0, RT_X) * 3 - e0;      // bytes of this group that lie inside the image
        if (valid <= 0) continue;
        unsigned w;
        if (KY) {
            const int first = max(by[2 * row] - y0, 0);
            const int* k = ky + row * KMAX;
            unsigned q[KY ? KY : 1];
#pragma unroll
            for (int t = 0; t < KY; ++t) q[t] = *(const unsigned*)(hrow + min(first + t, rows - 1) * ROWB + e0);
            int v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int ss = 1 << (PBITS - 1);
#pragma unroll
                for (int t = 0; t < KY; ++t) ss += (int)((q[t] >> (8 * j)) & 255u) * k[t];
                v[j] = clip8(ss);
            }
            w = pack4(v);
        } else {
            w = *(const unsigned*)(hrow + row * ROWB + e0);
        }
        uint8_t* po = out + ((long)oy * Wo + ox0) * 3 + e0;
        if (vec && valid >= 4) {
            *(unsigned*)po = w;
        } else {
            for (int j = 0; j < 4 && j < valid; ++j) po[j] = (uint8_t)(w >> (8 * j));
        }
    }
}

template <int KX, int KY>
int launch_resize(const uint8_t* src, uint8_t* dst, int N, int H, int W, int Ho, int Wo, const int* tx, const int* ty, hipStream_t st) {
    const int ksx = KX ? axis_ksize(W, Wo) : 0, ksy = KY ? axis_ksize(H, Ho) : 0;
    // rows a tile's vertical taps touch: (RT_Y - 1) * scale between the first and the last centre, a support and a rounding on either side
    const int max_rows = KY ? (int)ceil((RT_Y - 1) * ((double)H / (double)Ho) + 2.0 * axis_support(H, Ho)) + 2 : RT_Y;
    const size_t smem = (size_t)(RT_X * (KMAX + 1) + RT_Y * (KMAX + 2)) * sizeof(int) + (size_t)max_rows * ROWB;
    const int vec = ((long)Wo * 3) % 4 == 0 && ((uintptr_t)dst & 3) == 0;
    hipLaunchKernelGGL((k_resize_lanczos<KX, KY>), dim3(cdiv(Wo, RT_X), cdiv(Ho, RT_Y), N), dim3(256), smem, st, src, dst, H, W, Ho, Wo, tx, ty, ksx, ksy,
                       max_rows, vec);
    TCL_LAUNCH_RET();
}

// out [N,H,W,3] u8 from p [N,3,H,W] f32.  VEC: HW % 4 == 0 and p 16 B aligned -> a lane owns 4 consecutive pixels: three 16 B loads, 12 B out.
template <bool VEC>
__global__ __launch_bounds__(256) void k_frames_to_u8(const float* __restrict__ p, uint8_t* __restrict__ out, long N, long HW) {
#pragma clang fp contract(off)
    constexpr int V = VEC ? 4 : 1;
    const long per = HW / V, total = N * per;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const long n = g / per, i = (g - n * per) * V;
        const float* base = p + n * 3 * HW + i;
        float v[3][V];
        if constexpr (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 f = *(const float4*)(base + c * HW);
                v[c][0] = f.x; v[c][1] = f.y; v[c][2] = f.z; v[c][3] = f.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][0] = base[c * HW];
        }
        uint8_t b[3 * V];
#pragma unroll
        for (int j = 0; j < V; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float s = 255.f * v[c][j];
                b[3 * j + c] = (uint8_t)(int)fminf(fmaxf(s, 0.f), 255.f);      // fmaxf(NaN, 0) = 0
            }
        uint8_t* po = out + (n * HW + i) * 3;
        if constexpr (VEC) {
#pragma unroll
            for (int d = 0; d < 3; ++d)
                *(unsigned*)(po + 4 * d) = (unsigned)b[4 * d] | ((unsigned)b[4 * d + 1] << 8) | ((unsigned)b[4 * d + 2] << 16) | ((unsigned)b[4 * d + 3] << 24);
        } else {
            po[0] = b[0]; po[1] = b[1]; po[2] = b[2];
        }
    }
}

// out [N,3,H,W] f32 = u / denom from u [N,H,W,3] u8: one lane per pixel, three byte loads, three coalesced stores
__global__ __launch_bounds__(256) void k_u8_to_frames(const uint8_t* __restrict__ u, float* __restrict__ out, long N, long HW, float denom) {
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < N * HW; g += (long)gridDim.x * blockDim.x) {
        const long n = g / HW, i = g - n * HW;
        const uint8_t* pu = u + g * 3;
        const float r = (float)pu[0], gg = (float)pu[1], b = (float)pu[2];
        float* po = out + n * 3 * HW + i;
        po[0] = r / denom; po[HW] = gg / denom; po[2 * HW] = b / denom;
    }
}

}  // namespace

extern "C" {

size_t tcl_resize_lanczos_table_ints(int in, int out) {
    if (!axis_ok(in, out) || in == out) return 0;
    return (size_t)out * (2 + (size_t)axis_ksize(in, out));
}

int tcl_resize_lanczos_table(int in, int out, int* h_table) {
#pragma clang fp contract(off)
    TCL_CHECK_ARG(h_table && axis_ok(in, out) && in != out);
    // precompute_coeffs + normalize_coeffs_8bpc, operation for operation
    const double scale = (double)in / (double)out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    const double ss = 1.0 / filterscale;
    int* bounds = h_table;
    int* kk = h_table + 2 * (size_t)out;
    double w[2 * 6 + 1 + 2];                         // ksize <= 13
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        if (xmax > ksize) xmax = ksize;              // never true for these bounds; keeps w[] in range whatever the arguments
        double ww = 0.0;
        int x = 0;
        for (; x < xmax; ++x) {
            w[x] = lanczos3((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        for (x = 0; x < xmax; ++x)
            if (ww != 0.0) w[x] /= ww;
        for (; x < ksize; ++x) w[x] = 0.0;
        int* k = kk + (size_t)xx * ksize;
        for (x = 0; x < ksize; ++x) k[x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << PBITS)) : (int)(0.5 + w[x] * (1 << PBITS));
        bounds[2 * xx] = xmin; bounds[2 * xx + 1] = xmax;
    }
    return TCL_OK;
}

int tcl_resize_lanczos_u8(const void* src, void* dst, int N, int H, int W, int Ho, int Wo, const int* tx, const int* ty, hipStream_t st) {
    TCL_CHECK_ARG(src && dst && src != dst && N > 0 && N <= 65535 && axis_ok(H, Ho) && axis_ok(W, Wo));
    TCL_CHECK_ARG(3L * N * Ho * Wo < (1L << 31) && cdiv(Ho, RT_Y) <= 65535);
    TCL_CHECK_ARG((W == Wo || tx) && (H == Ho || ty));
    const uint8_t* s = (const uint8_t*)src;
    uint8_t* d = (uint8_t*)dst;
    if (W == Wo && H == Ho)                          // Image.resize to its own size is a copy
        return hipMemcpyAsync(d, s, 3L * N * H * W, hipMemcpyDeviceToDevice, st) == hipSuccess ? TCL_OK : TCL_ELAUNCH;
    const int kx = W == Wo ? 0 : (W <= Wo ? 7 : 13), ky = H == Ho ? 0 : (H <= Ho ? 7 : 13);
#define TCL_RESIZE_CASE(KX, KY) if (kx == KX && ky == KY) return launch_resize<KX, KY>(s, d, N, H, W, Ho, Wo, tx, ty, st)
    TCL_RESIZE_CASE(7, 7); TCL_RESIZE_CASE(7, 0); TCL_RESIZE_CASE(0, 7); TCL_RESIZE_CASE(7, 13); TCL_RESIZE_CASE(13, 7);
    TCL_RESIZE_CASE(13, 13); TCL_RESIZE_CASE(13, 0); TCL_RESIZE_CASE(0, 13);
#undef TCL_RESIZE_CASE
    return TCL_EINVAL;
}

int tcl_frames_to_u8(const float* frames, void* out, int N, int H, int W, hipStream_t st) {
    TCL_CHECK_ARG(frames && out && N > 0 && H > 0 && W > 0 && 3L * N * H * W < (1L << 31));
    const long hw = (long)H * W;
    if (hw % 4 == 0 && (((uintptr_t)frames & 15) | ((uintptr_t)out & 3)) == 0)
        hipLaunchKernelGGL(k_frames_to_u8<true>, dim3(stream_grid(N * (hw / 4))), dim3(256), 0, st, frames, (uint8_t*)out, (long)N, hw);
    else
        hipLaunchKernelGGL(k_frames_to_u8<false>, dim3(stream_grid(N * hw)), dim3(256), 0, st, frames, (uint8_t*)out, (long)N, hw);
    TCL_LAUNCH_RET();
}

int tcl_u8_to_frames_f32(const void* u8, float* out, int N, int H, int W, float denom, hipStream_t st) {
    TCL_CHECK_ARG(u8 && out && N > 0 && H > 0 && W > 0 && 3L * N * H * W < (1L << 31) && denom > 0.f);
    hipLaunchKernelGGL(k_u8_to_frames, dim3(stream_grid((long)N * H * W)), dim3(256), 0, st, (const uint8_t*)u8, out, (long)N, (long)H * W, denom);
    TCL_LAUNCH_RET();
}

}  // extern "C"
