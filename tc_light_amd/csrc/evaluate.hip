// warp-error-ssim, the temporal-consistency metric of evaluate.py (utils/evaluation/eval_utils.py:265-350: SaveWarpingImage with the RAFT flows,
// warp_flow / compute_fwdbwd_mask / structural_similarity).  Two kernels per batch of frame pairs:
//
// k_warp_mask (one thread per pixel of one pair i): bwd = past[i + 1], fwd = fut[i] (NCHW f32 planes as estimate_flows_raft returns them).  The
//   map m = bwd + (x, y) is put on cv2's 1/32-pixel grid (X = rint(m * 32), integer part X >> 5, fraction X & 31) and the 4 x 4 cubic taps
//   (A = -0.75, 2-D weight wy[i] * wx[j], taps outside the image read 0, summed row by row) are computed once and serve the 2 channels of fwd
//   (f2b, for the forward-backward mask) and the 3 colour channels of edit[i].  mask = |bwd + f2b| < 0.5 (|bwd| + |f2b|) + 0.5;
//   warped = u8(mask ? remap(edit[i]) : 0), target = u8(mask ? edit[i + 1] : 0), where u8 is numpy's cast on x86-64: truncate, keep 8 bits.
//   The whole float sequence is compiled without fma contraction, so the sums are the ones the CPU restatement (tests/eval_ref.py) makes.
// k_ssim_tile (one block per 64 x 32 tile of interior pixels, one wave per colour channel, one lane per column): the two u8 planes of the tile plus
//   a 3-pixel halo in LDS; each lane walks its column keeping the 7 x 7 window moments (sum x, sum y, sum x^2, sum y^2, sum xy) as exact integers
//   (sum x <= 12 495, 49 sum x^2 - (sum x)^2 < 2^31), so the per-pixel S, in f64, is the only rounding.  Each block writes its f64 sum of S into a
//   fixed slot; k_ssim_final adds the slots of a pair in a fixed order: no atomics, repeated runs are bit-identical.
#include "common.h"
#include "../../include/tclight_hip.h"

namespace {

// cv2's interpolateCubic at t = k / 32 (A = -0.75): not bicubic.h's cubic_w, whose last weight is the polynomial itself rather than 1 - the others
__device__ __forceinline__ void cv_cubic(int k, float c[4]) {
#pragma clang fp contract(off)
    const float A = -0.75f;
    const float t = (float)k * (1.f / 32.f);
    float x = t + 1.f;
    c[0] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
    c[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    x = 1.f - t;
    c[2] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// X = rint(m * 32) (round half to even); clamped far outside any frame so that the integer conversion is defined
__device__ __forceinline__ int cv_fixed(float m) {
    return (int)fminf(fmaxf(rintf(m * 32.f), -1.0e9f), 1.0e9f);
}

__global__ __launch_bounds__(256) void k_warp_mask(const uint8_t* __restrict__ edit, const float* __restrict__ fut, const float* __restrict__ past,
                                                   uint8_t* __restrict__ warped, uint8_t* __restrict__ target, int H, int W, int i0) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= W || y >= H) return;
    const int i = i0 + b;
    const long HW = (long)H * W, p = (long)y * W + x;
    const float* fw = fut + (long)i * 2 * HW;
    const float* bw = past + (long)(i + 1) * 2 * HW;
    const uint8_t* e0 = edit + (long)i * HW * 3;
    const float bx = bw[p], by = bw[HW + p];
    const int X = cv_fixed(bx + (float)x), Y = cv_fixed(by + (float)y);
    const int ix = (X >> 5) - 1, iy = (Y >> 5) - 1;
    float wx[4], wy[4];
    cv_cubic(X & 31, wx);
    cv_cubic(Y & 31, wy);
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};                 // f2b x, f2b y, R, G, B
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int yy = iy + r;
        const bool rv = yy >= 0 && yy < H;
        float row[5];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = ix + j;
            const float w = wy[r] * wx[j];
            // a tap outside the image loads the pixel itself and reads 0: no branch, so all 80 loads of the pixel are in flight together
            const bool ok = rv && xx >= 0 && xx < W;
            const long q = ok ? (long)yy * W + xx : p;
            float v[5] = {fw[q], fw[HW + q], (float)e0[q * 3], (float)e0[q * 3 + 1], (float)e0[q * 3 + 2]};
#pragma unroll
            for (int c = 0; c < 5; ++c) v[c] = ok ? v[c] : 0.f;
#pragma unroll
            for (int c = 0; c < 5; ++c) row[c] = j == 0 ? v[c] * w : row[c] + v[c] * w;
        }
#pragma unroll
        for (int c = 0; c < 5; ++c) acc[c] = acc[c] + row[c];
    }
    const float ex = bx + acc[0], ey = by + acc[1];
    const float lhs = sqrtf(ex * ex + ey * ey);
    const float n1 = sqrtf(bx * bx + by * by), n2 = sqrtf(acc[0] * acc[0] + acc[1] * acc[1]);
    const bool keep = lhs < 0.5f * (n1 + n2) + 0.5f;
    const uint8_t* e1 = e0 + HW * 3;
    const long o = ((long)b * HW + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        warped[o + c] = keep ? (uint8_t)((int)acc[2 + c] & 255) : (uint8_t)0;
        target[o + c] = keep ? e1[p * 3 + c] : (uint8_t)0;
    }
}

constexpr int TW = 64, TH = 32, LW = TW + 6, LH = TH + 6;   // interior tile, LDS tile with the 3-pixel halo
constexpr double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);

struct Mom { int x, y, xx, yy, xy; };

__device__ __forceinline__ Mom row_moments(const uint8_t* sx, const uint8_t* sy) {
    Mom m{0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const int u = sx[k], v = sy[k];
        m.x += u; m.y += v; m.xx += u * u; m.yy += v * v; m.xy += u * v;
    }
    return m;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(192) void k_ssim_tile(const uint8_t* __restrict__ X, const uint8_t* __restrict__ Y, double* __restrict__ part, int H, int W) {
    __shared__ uint8_t sx[3][LH][LW], sy[3][LH][LW];
    __shared__ double red[3];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int ox0 = 3 + blockIdx.x * TW, oy0 = 3 + blockIdx.y * TH;     // first interior pixel of the tile
    const long HW = (long)H * W;
    const uint8_t* xb = X + (long)b * HW * 3;
    const uint8_t* yb = Y + (long)b * HW * 3;
    // byte k of a tile row (LW pixels x 3 channels, contiguous in memory): thread tid loads bytes tid and tid + 192 of every row; bytes outside the
    // image load byte 0 and store 0 (no branch: the loads of all rows are in flight together)
    const int k1 = tid + 192, c0 = tid / 3, h0 = tid % 3, c1 = k1 / 3, h1 = k1 % 3;
    const bool in0 = ox0 - 3 + c0 < W, in1 = k1 < LW * 3 && ox0 - 3 + c1 < W;
#pragma unroll
    for (int r = 0; r < LH; ++r) {
        const bool rv = oy0 - 3 + r < H;
        const long row = ((long)(oy0 - 3 + r) * W + ox0 - 3) * 3;
        const long o0 = rv && in0 ? row + tid : 0, o1 = rv && in1 ? row + k1 : 0;
        const uint8_t u0 = xb[o0], v0 = yb[o0], u1 = xb[o1], v1 = yb[o1];
        sx[h0][r][c0] = rv && in0 ? u0 : 0; sy[h0][r][c0] = rv && in0 ? v0 : 0;
        if (k1 < LW * 3) { sx[h1][r][c1] = rv && in1 ? u1 : 0; sy[h1][r][c1] = rv && in1 ? v1 : 0; }
    }
    __syncthreads();
    const int ch = tid >> 6, c = tid & 63;
    const bool colv = ox0 + c < W - 3;
    const int rows = min(TH, H - 3 - oy0);                             // interior rows of this tile
    Mom s{0, 0, 0, 0, 0};
    double acc = 0.0;
    if (colv) {
        for (int r = 0; r < 6; ++r) {
            const Mom m = row_moments(&sx[ch][r][c], &sy[ch][r][c]);
            s.x += m.x; s.y += m.y; s.xx += m.xx; s.yy += m.yy; s.xy += m.xy;
        }
        for (int r = 0; r < rows; ++r) {
            const Mom a = row_moments(&sx[ch][r + 6][c], &sy[ch][r + 6][c]);
            s.x += a.x; s.y += a.y; s.xx += a.xx; s.yy += a.yy; s.xy += a.xy;
            // S = ((2 mx my + C1)(2 cxy + C2)) / ((mx^2 + my^2 + C1)(vx + vy + C2)) with means over 49 and the 49/48 covariance: every factor
            // times 49^2 or 49 * 48 is an integer plus a constant
            const int sxsy = s.x * s.y;
            const double n1 = (double)(2 * sxsy) + 2401.0 * C1;
            const double n2 = (double)(2 * (49 * s.xy - sxsy)) + 2352.0 * C2;
            const double d1 = (double)(s.x * s.x + s.y * s.y) + 2401.0 * C1;
            const double d2 = (double)((49 * s.xx - s.x * s.x) + (49 * s.yy - s.y * s.y)) + 2352.0 * C2;
            acc += (n1 * n2) / (d1 * d2);
            const Mom d = row_moments(&sx[ch][r][c], &sy[ch][r][c]);
            s.x -= d.x; s.y -= d.y; s.xx -= d.xx; s.yy -= d.yy; s.xy -= d.xy;
        }
    }
    acc = wave_sum_f64(acc);
    if (c == 0) red[ch] = acc;
    __syncthreads();
    if (tid == 0) part[((long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + red[2];
}

__global__ __launch_bounds__(256) void k_ssim_final(const double* __restrict__ part, int nblk, double inv_count, double* __restrict__ out) {
    __shared__ double red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    double v = 0.0;
    for (int k = tid; k < nblk; k += 256) v += part[(long)b * nblk + k];
    v = wave_sum_f64(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) out[b] = (((red[0] + red[1]) + red[2]) + red[3]) * inv_count;
}

inline int ssim_blocks(int H, int W) { return cdiv(W - 6, TW) * cdiv(H - 6, TH); }

}  // namespace

extern "C" {

int tcl_eval_warp_mask_u8(const void* edit, const float* fut, const float* past, void* warped, void* target, int N, int H, int W, int i0, int B,
                          hipStream_t st) {
    TCL_CHECK_ARG(edit && fut && past && warped && target && H > 0 && W > 0 && B > 0 && i0 >= 0 && i0 + B <= N - 1);
    TCL_CHECK_ARG(B <= 65535 && (long)H * W < (1L << 30));
    hipLaunchKernelGGL(k_warp_mask, dim3(cdiv(W, 64), cdiv(H, 4), B), dim3(256), 0, st, (const uint8_t*)edit, fut, past, (uint8_t*)warped,
                       (uint8_t*)target, H, W, i0);
    TCL_LAUNCH_RET();
}

size_t tcl_eval_ssim_workspace_bytes(int B, int H, int W) {
    return (H >= 7 && W >= 7 && B > 0) ? (size_t)B * ssim_blocks(H, W) * sizeof(double) : 0;
}

int tcl_eval_ssim_u8(const void* x, const void* y, double* out, int B, int H, int W, void* ws, hipStream_t st) {
    TCL_CHECK_ARG(x && y && out && ws && B > 0 && B <= 65535 && H >= 7 && W >= 7 && (long)H * W < (1L << 30));
    double* part = (double*)ws;
    const dim3 grid(cdiv(W - 6, TW), cdiv(H - 6, TH), B);
    hipLaunchKernelGGL(k_ssim_tile, grid, dim3(192), 0, st, (const uint8_t*)x, (const uint8_t*)y, part, H, W);
    hipLaunchKernelGGL(k_ssim_final, dim3(B), dim3(256), 0, st, (const double*)part, ssim_blocks(H, W), 1.0 / (3.0 * (H - 6) * (W - 6)), out);
    TCL_LAUNCH_RET();
}

}  // extern "C"
