// generation.detail_transfer: the relit frames keep their low frequencies (the new light), the source frames give back the high ones (texture,
// small text, faces) that the 8x VAE and the denoise softened.  Per frame, independent of every other frame; runs once, behind stage 1 / 2.
//   add:    D = S - R;  P = D - G(D);  O = clamp(R + (b m) P, 0, 1)                       (luma: P = Y(D) - G(Y(D)), the same P for the three channels)
//   ratio:  T = S (G(R) + e) / (G(S) + e), e = 1/255;  O = clamp(R + (b m)(T - R), 0, 1)  (luma: the ratio of G(Y(R)) and G(Y(S)))
// G is a separable Gaussian of radius r <= 48 with reflected borders (index -i -> i, L-1+i -> L-1-i: the edge sample is not repeated).
// Two launches over all N frames, the intermediate in an f32 workspace:
//   k_detail_rows   one block per 256-pixel row segment: the planes to blur (D_c | Y(D) | R_c, S_c | Y(R), Y(S)) of the segment and its halo go to LDS,
//                   every lane sums the 2r+1 taps of its pixel in ascending tap order with fmaf from 0 and stores to the workspace;
//   k_detail_cols   one block per 64 x 32 tile of one blurred group: rows y0-r .. y0+31+r of the workspace go to LDS (a lane's loads are independent of one
//                   another: all in flight before the first LDS store), then per pixel the same tap sum down the column and the combine, which reads S, R
//                   and m once and stores O once.
// HBM traffic per pixel (add, rgb): 24 B in + 12 B workspace out, then 12 B workspace (+ halo rows, mostly L2 hits) + 24 B in + 12 B out.
// The taps travel as a kernel argument (at most 97 floats): every tap read is a scalar load of the kernarg segment, no device table to upload.
#include "common.h"
#include "../../include/tclight_hip.h"

namespace {

constexpr int SEG = TCL_DETAIL_ROW_SEG, TW = TCL_DETAIL_TILE_W, TH = TCL_DETAIL_TILE_H, RMAX = TCL_DETAIL_MAX_RADIUS;
static_assert(SEG == 256 && TW == 64 && TH % 4 == 0, "the kernels below are written for 256 lanes: one row segment, or 64 columns x 4 row phases");

struct DetailTaps { float w[2 * RMAX + 1]; };

__device__ __forceinline__ int reflect(int i, int L) {          // -r <= i <= L-1+r with r <= L-1: one reflection lands inside
    i = i < 0 ? -i : i;
    return i > L - 1 ? 2 * (L - 1) - i : i;
}

__device__ __forceinline__ float luma(float r, float g, float b) {
    return fmaf(0.114f, b, fmaf(0.587f, g, 0.299f * r));
}

// planes the rows pass leaves per frame: add 3 (rgb) | 1 (luma), ratio 6 (G(R_c), then G(S_c), c-major pairs) | 2
__host__ __device__ constexpr int n_planes(int mode, int lum) { return (mode == TCL_DETAIL_RATIO ? 2 : 1) * (lum ? 1 : 3); }

// ws [N, P, H, W].  Plane order: add rgb: D_0 D_1 D_2; add luma: Y(D); ratio rgb: R_0 S_0 R_1 S_1 R_2 S_2; ratio luma: Y(R) Y(S).
template <int MODE, int LUMA>
__global__ __launch_bounds__(SEG) void k_detail_rows(const float* __restrict__ src, const float* __restrict__ relit, float* __restrict__ ws, int H, int W,
                                                     DetailTaps taps, int r) {
#pragma clang fp contract(off)
    constexpr int P = n_planes(MODE, LUMA);
    __shared__ float tile[P][SEG + 2 * RMAX];
    const int x0 = blockIdx.x * SEG, y = blockIdx.y;
    const long hw = (long)H * W, n = blockIdx.z;
    const float* ps = src + n * 3 * hw + (long)y * W;
    const float* pr = relit + n * 3 * hw + (long)y * W;
    const int need = min(SEG, W - x0) + 2 * r;                  // LDS entries the segment's pixels read
    for (int i = threadIdx.x; i < need; i += SEG) {
        const int gx = reflect(x0 - r + i, W);                  // x0 - r + i <= W-1+r by `need`: always inside, no guard around a load
        float s[3], q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { s[c] = ps[c * hw + gx]; q[c] = pr[c * hw + gx]; }
        if constexpr (MODE == TCL_DETAIL_ADD) {
            float d[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = s[c] - q[c];
            if constexpr (LUMA) {
                tile[0][i] = luma(d[0], d[1], d[2]);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) tile[c][i] = d[c];
            }
        } else if constexpr (LUMA) {
            tile[0][i] = luma(q[0], q[1], q[2]);
            tile[1][i] = luma(s[0], s[1], s[2]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) { tile[2 * c][i] = q[c]; tile[2 * c + 1][i] = s[c]; }
        }
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    float acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = 0.f;
    for (int k = 0; k <= 2 * r; ++k) {
        const float w = taps.w[k];
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p] = fmaf(w, tile[p][threadIdx.x + k], acc[p]);
    }
    float* po = ws + (n * P * H + y) * W + x;
#pragma unroll
    for (int p = 0; p < P; ++p) po[p * hw] = acc[p];
}

// One block: the tile (x0 .. x0+63) x (y0 .. y0+31) of one group of one frame.  rgb: group = channel (grid.z = 3 N); luma: one group (grid.z = N), the
// combine walks the three channels.  LDS: PB planes x (32 + 2r) rows x 64 floats, at most 64 KB (dynamic).
template <int MODE, int LUMA, int MASK>
__global__ __launch_bounds__(256) void k_detail_cols(const float* __restrict__ src, const float* __restrict__ relit, const float* __restrict__ mask,
                                                     const float* __restrict__ ws, float* __restrict__ out, int H, int W, DetailTaps taps, int r,
                                                     float blend) {
#pragma clang fp contract(off)
    constexpr int PB = MODE == TCL_DETAIL_RATIO ? 2 : 1, G = LUMA ? 1 : 3, P = PB * G;
    extern __shared__ __attribute__((aligned(16))) float lds[];          // [PB][TH + 2r][TW]
    const int tx = threadIdx.x & (TW - 1), tq = threadIdx.x >> 6;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const long hw = (long)H * W, n = blockIdx.z / G;
    const int g = blockIdx.z % G;
    const int rows = min(TH, H - y0) + 2 * r;
    const int xc = min(x0 + tx, W - 1);                         // a column past the edge loads the last one again and stores nothing
    const float* pw = ws + (n * P + (long)g * PB) * hw + xc;
#pragma unroll 4
    for (int i = tq; i < rows; i += 4) {
        const long gy = reflect(y0 - r + i, H);
#pragma unroll
        for (int p = 0; p < PB; ++p) lds[(p * (TH + 2 * r) + i) * TW + tx] = pw[p * hw + gy * W];
    }
    __syncthreads();
    if (x0 + tx >= W) return;
    constexpr float eps = 1.f / 255.f;
    for (int j = tq; j < TH && y0 + j < H; j += 4) {
        const long px = (long)(y0 + j) * W + x0 + tx;
        constexpr int NC = LUMA ? 3 : 1;
        float s[NC], q[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const long e = (n * 3 + (LUMA ? c : g)) * hw + px;
            s[c] = src[e]; q[c] = relit[e];
        }
        float bm = blend;
        if (MASK) bm = blend * mask[n * hw + px];
        float acc[PB];
#pragma unroll
        for (int p = 0; p < PB; ++p) acc[p] = 0.f;
        for (int k = 0; k <= 2 * r; ++k) {
            const float w = taps.w[k];
#pragma unroll
            for (int p = 0; p < PB; ++p) acc[p] = fmaf(w, lds[(p * (TH + 2 * r) + j + k) * TW + tx], acc[p]);
        }
        float o[NC];
        if constexpr (MODE == TCL_DETAIL_ADD) {
            float d0[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) d0[c] = s[c] - q[c];
            float hp;
            if constexpr (LUMA) hp = luma(d0[0], d0[1], d0[2]) - acc[0];
            else hp = d0[0] - acc[0];
            const float t = bm * hp;
#pragma unroll
            for (int c = 0; c < NC; ++c) o[c] = q[c] + t;
        } else {
            const float num = acc[0] + eps, den = acc[PB - 1] + eps;
            const float ratio = num / den;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float T = s[c] * ratio;
                const float d = T - q[c];
                const float t = bm * d;
                o[c] = q[c] + t;
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) out[(n * 3 + (LUMA ? c : g)) * hw + px] = fminf(fmaxf(o[c], 0.f), 1.f);
    }
}

template <int MODE, int LUMA>
int launch(const float* src, const float* relit, const float* mask, float* out, int N, int H, int W, const DetailTaps& taps, int r, float blend,
           float* ws, hipStream_t st) {
    constexpr int PB = MODE == TCL_DETAIL_RATIO ? 2 : 1, G = LUMA ? 1 : 3;
    hipLaunchKernelGGL((k_detail_rows<MODE, LUMA>), dim3(cdiv(W, SEG), H, N), dim3(SEG), 0, st, src, relit, ws, H, W, taps, r);
    const dim3 grid(cdiv(W, TW), cdiv(H, TH), N * G);
    const size_t lds = (size_t)PB * (TH + 2 * r) * TW * sizeof(float);
    if (mask)
        hipLaunchKernelGGL((k_detail_cols<MODE, LUMA, 1>), grid, dim3(256), lds, st, src, relit, mask, ws, out, H, W, taps, r, blend);
    else
        hipLaunchKernelGGL((k_detail_cols<MODE, LUMA, 0>), grid, dim3(256), lds, st, src, relit, mask, ws, out, H, W, taps, r, blend);
    TCL_LAUNCH_RET();
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" {

size_t tcl_detail_transfer_workspace_bytes(int N, int H, int W, int mode, int luma) {
    if (N <= 0 || H <= 0 || W <= 0 || (mode != TCL_DETAIL_ADD && mode != TCL_DETAIL_RATIO) || (luma != 0 && luma != 1)) return 0;
    return (size_t)N * n_planes(mode, luma) * H * W * sizeof(float);
}

int tcl_detail_transfer_f32(const float* src, const float* relit, const float* mask, float* out, int N, int H, int W, const float* h_taps, int n_taps,
                            int radius, int mode, int luma, float blend, void* ws, long ws_bytes, hipStream_t st) {
    TCL_CHECK_ARG(src && relit && out && h_taps && ws && N > 0 && H > 0 && W > 0);
    TCL_CHECK_ARG(radius >= 1 && radius <= RMAX && n_taps == 2 * radius + 1 && radius < H && radius < W);
    TCL_CHECK_ARG((mode == TCL_DETAIL_ADD || mode == TCL_DETAIL_RATIO) && (luma == 0 || luma == 1) && blend >= 0.f && blend <= 1.f);      // NaN fails both
    TCL_CHECK_ARG(N <= 65535 / 3 && H <= 65535);                // grid.y = H rows, grid.z = 3 N groups
    const size_t need = tcl_detail_transfer_workspace_bytes(N, H, W, mode, luma), img = (size_t)N * 3 * H * W * sizeof(float);
    TCL_CHECK_ARG(ws_bytes >= 0 && (size_t)ws_bytes >= need && ((uintptr_t)ws & 3) == 0);
    TCL_CHECK_ARG(!overlap(out, img, src, img) && !overlap(out, img, relit, img) && !overlap(out, img, ws, need) && !overlap(ws, need, src, img) &&
                  !overlap(ws, need, relit, img));
    if (mask) TCL_CHECK_ARG(!overlap(out, img, mask, img / 3) && !overlap(ws, need, mask, img / 3));
    DetailTaps taps;
    for (int k = 0; k < 2 * RMAX + 1; ++k) taps.w[k] = k < n_taps ? h_taps[k] : 0.f;
    for (int k = 0; k < n_taps; ++k) TCL_CHECK_ARG(taps.w[k] >= 0.f && taps.w[k] <= 1.f);      // a Gaussian's; NaN fails
    float* w = (float*)ws;
    if (mode == TCL_DETAIL_ADD)
        return luma ? launch<TCL_DETAIL_ADD, 1>(src, relit, mask, out, N, H, W, taps, radius, blend, w, st)
                    : launch<TCL_DETAIL_ADD, 0>(src, relit, mask, out, N, H, W, taps, radius, blend, w, st);
    return luma ? launch<TCL_DETAIL_RATIO, 1>(src, relit, mask, out, N, H, W, taps, radius, blend, w, st)
                : launch<TCL_DETAIL_RATIO, 0>(src, relit, mask, out, N, H, W, taps, radius, blend, w, st);
}

}  // extern "C"
