// generation.fullres: the relight applied to the source's own pixels (the fast guided filter, He & Sun 2015).  A relit frame is close to a smooth
// per-pixel gain / offset on its source frame, so the model  R ~ a G + b  is fitted in every clipped (2r+1)^2 window of the working size (G: the
// guide -- the source channel itself, or the source's luminance), the fields a, b are box-averaged once more, upsampled bilinearly and applied to
// the native uint8 source frame.  Per frame, independent of every other frame.
//   tcl_guided_fit_f32   four launches over all N frames, everything between them in the f32 workspace:
//     k_moment_rows   one block per 256-pixel row segment: g = G - 0.5, q = R - 0.5 of the segment and its halo go to LDS, every lane sums g, q, g g, g q
//                     over its clipped window in ascending x and stores the four row SUMS per channel (luma: g, g g once);
//     k_solve_cols    one block per 64 x 32 tile of one channel: per pixel the same sums down the clipped column in ascending y (a lane's loads of one
//                     trip are independent: four in flight, eight under luma; hipcc waits per trip although the trips are unrolled), the division by
//                     the true pixel count, the solve;
//     k_box_rows / k_box_cols   the second box mean, of a and b: the same two passes on the six planes.
//     The moments are CENTRED at 0.5 (the inputs live in [0,1]): var and cov are differences of numbers <= 1/4 instead of <= 1, which is what the
//     derived bound (tests/fullres_refs.py) charges for; there is no second pass over the data.
//   tcl_guided_apply_u8  one launch: a lane owns four neighbouring output pixels of a row; its 12 source bytes, then per pixel the 24 field taps
//                     (2 fields x 3 channels x 4 corners) are loaded before the first of them is used, then the bilinear blends, a S + 255 b, round to
//                     nearest even, clamp, and 12 bytes are stored (three dwords where the rows are dword-aligned, bytes otherwise).  HBM traffic: 3 B in + 3 B out per output pixel; the fields are L2 hits.
#include "common.h"
#include "../../include/tclight_hip.h"

namespace {

constexpr int SEG = TCL_GUIDED_ROW_SEG, TW = TCL_GUIDED_TILE_W, TH = TCL_GUIDED_TILE_H, RMAX = TCL_GUIDED_MAX_RADIUS, WSP = TCL_GUIDED_WS_PLANES;
static_assert(SEG == 256 && TW == 64 && TH % 4 == 0 && WSP == 18, "256 lanes: one row segment, or 64 columns x 4 row phases; 12 + 6 planes");

__device__ __forceinline__ float luma(float r, float g, float b) {      // detail.hip's: the same weights and sequence
    return fmaf(0.114f, b, fmaf(0.587f, g, 0.299f * r));
}

// row sums of the centred moments.  mom [N, P, h, w] with P = 12 (rgb: per channel c the planes 4c + (g, q, gg, gq)) or 8 (luma: g, gg, then q_c, gq_c).
template <int LUMA>
__global__ __launch_bounds__(SEG) void k_moment_rows(const float* __restrict__ src, const float* __restrict__ relit, float* __restrict__ mom, int h, int w,
                                                     int r) {
#pragma clang fp contract(off)
    constexpr int G = LUMA ? 1 : 3, P = LUMA ? 8 : 12;
    __shared__ float tg[G][SEG + 2 * RMAX], tq[3][SEG + 2 * RMAX];
    const int x0 = blockIdx.x * SEG, y = blockIdx.y;
    const long hw = (long)h * w, n = blockIdx.z;
    const float* ps = src + n * 3 * hw + (long)y * w;
    const float* pr = relit + n * 3 * hw + (long)y * w;
    const int need = min(SEG, w - x0) + 2 * r;
    for (int i = threadIdx.x; i < need; i += SEG) {
        const int gx = min(max(x0 - r + i, 0), w - 1);          // outside the image: the edge pixel again, which no clipped window reads
        float s[3], q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { s[c] = ps[c * hw + gx]; q[c] = pr[c * hw + gx]; }
        if constexpr (LUMA) {
            tg[0][i] = luma(s[0], s[1], s[2]) - 0.5f;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) tg[c][i] = s[c] - 0.5f;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) tq[c][i] = q[c] - 0.5f;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    const int ka = max(x - r, 0) - (x0 - r), kb = min(x + r, w - 1) - (x0 - r);      // LDS indices of the clipped window
    float sg[G], sgg[G], sq[3], sgq[3];
#pragma unroll
    for (int c = 0; c < G; ++c) sg[c] = sgg[c] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) sq[c] = sgq[c] = 0.f;
    for (int k = ka; k <= kb; ++k) {
        float g[G];
#pragma unroll
        for (int c = 0; c < G; ++c) {
            g[c] = tg[c][k];
            sg[c] = sg[c] + g[c];
            sgg[c] = sgg[c] + g[c] * g[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float q = tq[c][k];
            sq[c] = sq[c] + q;
            sgq[c] = sgq[c] + g[LUMA ? 0 : c] * q;
        }
    }
    float* po = mom + (n * P * h + y) * w + x;
    if constexpr (LUMA) {
        po[0] = sg[0]; po[hw] = sgg[0];
#pragma unroll
        for (int c = 0; c < 3; ++c) { po[(2 + 2 * c) * hw] = sq[c]; po[(3 + 2 * c) * hw] = sgq[c]; }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) { po[(4 * c) * hw] = sg[c]; po[(4 * c + 1) * hw] = sq[c]; po[(4 * c + 2) * hw] = sgg[c]; po[(4 * c + 3) * hw] = sgq[c]; }
    }
}

// the pixel count of the clipped window, exact in f32 (at most 129^2)
__device__ __forceinline__ float window_count(int x, int y, int w, int h, int r) {
    return (float)((min(x + r, w - 1) - max(x - r, 0) + 1) * (min(y + r, h - 1) - max(y - r, 0) + 1));
}

__device__ __forceinline__ void solve(float tg, float tq, float tgg, float tgq, float cnt, float eps, float& a, float& b) {
#pragma clang fp contract(off)
    const float mg = tg / cnt, mq = tq / cnt, mgg = tgg / cnt, mgq = tgq / cnt;
    const float var = fmaxf(mgg - mg * mg, 0.f), cov = mgq - mg * mq;
    a = cov / (var + eps);
    b = ((mq - a * mg) + 0.5f) - 0.5f * a;                      // back from the centred model: R = a G + (mq' - a mg' + 0.5 - 0.5 a)
}

// column sums of the moments + the solve.  ab [N, 6, h, w]: plane 2c = a_c, 2c + 1 = b_c.  grid (tiles across x 3 channels | tiles across, tiles down, N).
template <int LUMA>
__global__ __launch_bounds__(256) void k_solve_cols(const float* __restrict__ mom, float* __restrict__ ab, int h, int w, int r, float eps) {
#pragma clang fp contract(off)
    constexpr int P = LUMA ? 8 : 12;
    const int tx = threadIdx.x & (TW - 1), tq = threadIdx.x >> 6;
    const int tiles = (w + TW - 1) / TW;
    const int c0 = LUMA ? 0 : blockIdx.x / tiles;                // rgb: this block's channel
    const int x = (LUMA ? blockIdx.x : blockIdx.x % tiles) * TW + tx, y0 = blockIdx.y * TH;
    const long hw = (long)h * w, n = blockIdx.z;
    if (x >= w) return;
    const float* pm = mom + n * P * hw + x;
    float* pa = ab + n * 6 * hw + x;
    for (int j = tq; j < TH && y0 + j < h; j += 4) {
        const int y = y0 + j, ya = max(y - r, 0), yb = min(y + r, h - 1);
        const float cnt = window_count(x, y, w, h, r);
        if constexpr (LUMA) {
            float t[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) t[p] = 0.f;
#pragma unroll 4
            for (int yy = ya; yy <= yb; ++yy) {
#pragma unroll
                for (int p = 0; p < 8; ++p) t[p] = t[p] + pm[p * hw + (long)yy * w];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float a, b;
                solve(t[0], t[2 + 2 * c], t[1], t[3 + 2 * c], cnt, eps, a, b);
                pa[(2 * c) * hw + (long)y * w] = a;
                pa[(2 * c + 1) * hw + (long)y * w] = b;
            }
        } else {
            float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int yy = ya; yy <= yb; ++yy) {
#pragma unroll
                for (int p = 0; p < 4; ++p) t[p] = t[p] + pm[(4 * c0 + p) * hw + (long)yy * w];
            }
            float a, b;
            solve(t[0], t[1], t[2], t[3], cnt, eps, a, b);
            pa[(2 * c0) * hw + (long)y * w] = a;
            pa[(2 * c0 + 1) * hw + (long)y * w] = b;
        }
    }
}

// row sums of a and b: in, out [N, 6, h, w].  grid (segments x 6 planes, h, N).
__global__ __launch_bounds__(SEG) void k_box_rows(const float* __restrict__ in, float* __restrict__ out, int h, int w, int r) {
#pragma clang fp contract(off)
    __shared__ float t[SEG + 2 * RMAX];
    const int segs = (w + SEG - 1) / SEG;
    const int x0 = (blockIdx.x % segs) * SEG, p = blockIdx.x / segs, y = blockIdx.y;
    const long row = (((long)blockIdx.z * 6 + p) * h + y) * w;
    const int need = min(SEG, w - x0) + 2 * r;
    for (int i = threadIdx.x; i < need; i += SEG) t[i] = in[row + min(max(x0 - r + i, 0), w - 1)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    const int ka = max(x - r, 0) - (x0 - r), kb = min(x + r, w - 1) - (x0 - r);
    float s = 0.f;
    for (int k = ka; k <= kb; ++k) s = s + t[k];
    out[row + x] = s;
}

// column sums of the row sums of a and b, divided by the pixel count.  in [N, 6, h, w] -> abar, bbar [N, 3, h, w].  grid (tiles across x 6 planes, tiles down, N).
__global__ __launch_bounds__(256) void k_box_cols(const float* __restrict__ in, float* __restrict__ abar, float* __restrict__ bbar, int h, int w, int r) {
#pragma clang fp contract(off)
    const int tx = threadIdx.x & (TW - 1), tq = threadIdx.x >> 6;
    const int tiles = (w + TW - 1) / TW;
    const int p = blockIdx.x / tiles, x = (blockIdx.x % tiles) * TW + tx, y0 = blockIdx.y * TH;
    const long hw = (long)h * w, n = blockIdx.z;
    if (x >= w) return;
    const float* pi = in + (n * 6 + p) * hw + x;
    float* po = ((p & 1) ? bbar : abar) + (n * 3 + (p >> 1)) * hw + x;
    for (int j = tq; j < TH && y0 + j < h; j += 4) {
        const int y = y0 + j, ya = max(y - r, 0), yb = min(y + r, h - 1);
        float s = 0.f;
#pragma unroll 8
        for (int yy = ya; yy <= yb; ++yy) s = s + pi[(long)yy * w];
        po[(long)y * w] = s / window_count(x, y, w, h, r);
    }
}

// One lane: the output pixels X0 .. X0+3 of row Y of frame n.  VEC: Wc % 4 == 0 and 4-byte aligned bases, so the 12 bytes are three aligned dwords.
template <int VEC>
__global__ __launch_bounds__(256) void k_guided_apply(const float* __restrict__ abar, const float* __restrict__ bbar, const unsigned char* __restrict__ src,
                                                      unsigned char* __restrict__ out, int h, int w, int Hc, int Wc, float sx, float sy) {
#pragma clang fp contract(off)
    const int X0 = (blockIdx.x * 256 + threadIdx.x) * 4, Y = blockIdx.y;
    if (X0 >= Wc) return;
    const long hw = (long)h * w, n = blockIdx.z;
    const long base = ((n * Hc + Y) * Wc + X0) * 3;
    float v = ((float)Y + 0.5f) * sy - 0.5f;
    v = fminf(fmaxf(v, 0.f), (float)(h - 1));
    const int y0 = (int)v, y1 = min(y0 + 1, h - 1);
    const float fy = v - (float)y0;
    int xa[4], xb[4];
    float fx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float u = ((float)(X0 + i) + 0.5f) * sx - 0.5f;         // a pixel past the row's end: a valid field address all the same, never stored
        u = fminf(fmaxf(u, 0.f), (float)(w - 1));
        xa[i] = (int)u; xb[i] = min(xa[i] + 1, w - 1);
        fx[i] = u - (float)xa[i];
    }
    unsigned char s8[12];
    const int nb = min(4, Wc - X0) * 3;                           // bytes of this lane inside the row
    if constexpr (VEC) {
        const unsigned int* p = reinterpret_cast<const unsigned int*>(src + base);
        const unsigned int d0 = p[0], d1 = p[1], d2 = p[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) { s8[k] = (d0 >> (8 * k)) & 255u; s8[4 + k] = (d1 >> (8 * k)) & 255u; s8[8 + k] = (d2 >> (8 * k)) & 255u; }
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) s8[k] = src[base + min(k, nb - 1)];      // past the row's end: the lane's last byte again
    }
    unsigned int o8[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float fa[3][4], fb[3][4];                                 // the 24 taps of one pixel: all issued before the first is used
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long o0 = (n * 3 + c) * hw + (long)y0 * w, o1 = (n * 3 + c) * hw + (long)y1 * w;
            fa[c][0] = abar[o0 + xa[i]]; fa[c][1] = abar[o0 + xb[i]]; fa[c][2] = abar[o1 + xa[i]]; fa[c][3] = abar[o1 + xb[i]];
            fb[c][0] = bbar[o0 + xa[i]]; fb[c][1] = bbar[o0 + xb[i]]; fb[c][2] = bbar[o1 + xa[i]]; fb[c][3] = bbar[o1 + xb[i]];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float at = fa[c][0] + fx[i] * (fa[c][1] - fa[c][0]), ab = fa[c][2] + fx[i] * (fa[c][3] - fa[c][2]);
            const float bt = fb[c][0] + fx[i] * (fb[c][1] - fb[c][0]), bb = fb[c][2] + fx[i] * (fb[c][3] - fb[c][2]);
            const float A = at + fy * (ab - at), B = bt + fy * (bb - bt);
            const float o = A * (float)s8[3 * i + c] + 255.f * B;
            o8[3 * i + c] = (unsigned int)fminf(fmaxf(rintf(o), 0.f), 255.f);      // NaN (from a NaN field) -> fmaxf gives 0
        }
    }
    if constexpr (VEC) {
        unsigned int* p = reinterpret_cast<unsigned int*>(out + base);
        p[0] = o8[0] | (o8[1] << 8) | (o8[2] << 16) | (o8[3] << 24);
        p[1] = o8[4] | (o8[5] << 8) | (o8[6] << 16) | (o8[7] << 24);
        p[2] = o8[8] | (o8[9] << 8) | (o8[10] << 16) | (o8[11] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < nb) out[base + k] = (unsigned char)o8[k];
    }
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

constexpr long LIM = 2147483647L;

}  // namespace

extern "C" {

size_t tcl_guided_workspace_bytes(int N, int h, int w) {
    if (N <= 0 || N > 65535 || h <= 0 || w <= 0 || h > 65535 || (long)N * WSP * h * w > LIM) return 0;
    return (size_t)N * WSP * h * w * sizeof(float);
}

int tcl_guided_fit_f32(const float* src, const float* relit, float* abar, float* bbar, int N, int h, int w, int radius, float eps, int luma, void* ws,
                       long ws_bytes, hipStream_t st) {
    TCL_CHECK_ARG(src && relit && abar && bbar && ws && N >= 1 && N <= 65535 && h >= 1 && w >= 1 && h <= 65535);
    TCL_CHECK_ARG(radius >= 1 && radius <= RMAX && (luma == 0 || luma == 1) && eps >= 1e-4f && eps <= 1.f);      // NaN fails both
    TCL_CHECK_ARG((long)N * WSP * h * w <= LIM);
    const size_t need = tcl_guided_workspace_bytes(N, h, w), img = (size_t)N * 3 * h * w * sizeof(float);
    TCL_CHECK_ARG(need > 0 && ws_bytes >= 0 && (size_t)ws_bytes >= need && ((uintptr_t)ws & 3) == 0);
    TCL_CHECK_ARG(!overlap(abar, img, bbar, img) && !overlap(ws, need, src, img) && !overlap(ws, need, relit, img));
    for (const float* o : {abar, bbar})
        TCL_CHECK_ARG(!overlap(o, img, src, img) && !overlap(o, img, relit, img) && !overlap(o, img, ws, need));
    float* mom = (float*)ws;                                   // [N, 12, h, w] row sums of the moments, then [N, 6, h, w] row sums of a, b
    float* ab = mom + (size_t)N * 12 * h * w;                  // [N, 6, h, w] a, b
    const int segs = cdiv(w, SEG), tiles = cdiv(w, TW), down = cdiv(h, TH);
    if (luma) {
        hipLaunchKernelGGL(k_moment_rows<1>, dim3(segs, h, N), dim3(SEG), 0, st, src, relit, mom, h, w, radius);
        hipLaunchKernelGGL(k_solve_cols<1>, dim3(tiles, down, N), dim3(256), 0, st, mom, ab, h, w, radius, eps);
    } else {
        hipLaunchKernelGGL(k_moment_rows<0>, dim3(segs, h, N), dim3(SEG), 0, st, src, relit, mom, h, w, radius);
        hipLaunchKernelGGL(k_solve_cols<0>, dim3(tiles * 3, down, N), dim3(256), 0, st, mom, ab, h, w, radius, eps);
    }
    hipLaunchKernelGGL(k_box_rows, dim3(segs * 6, h, N), dim3(SEG), 0, st, ab, mom, h, w, radius);
    hipLaunchKernelGGL(k_box_cols, dim3(tiles * 6, down, N), dim3(256), 0, st, mom, abar, bbar, h, w, radius);
    TCL_LAUNCH_RET();
}

int tcl_guided_apply_u8(const float* abar, const float* bbar, const unsigned char* src, unsigned char* out, int N, int h, int w, int Hc, int Wc,
                        hipStream_t st) {
    TCL_CHECK_ARG(abar && bbar && src && out && N >= 1 && N <= 65535 && h >= 1 && w >= 1 && Hc >= 1 && Wc >= 1 && Hc <= 65535);
    TCL_CHECK_ARG((long)N * 3 * h * w <= LIM && (long)N * 3 * Hc * Wc <= LIM);
    const size_t fld = (size_t)N * 3 * h * w * sizeof(float), img = (size_t)N * 3 * Hc * Wc;
    TCL_CHECK_ARG(!overlap(out, img, src, img) && !overlap(out, img, abar, fld) && !overlap(out, img, bbar, fld));
    const float sx = (float)w / (float)Wc, sy = (float)h / (float)Hc;
    const dim3 grid(cdiv(cdiv(Wc, 4), 256), Hc, N);
    if (Wc % 4 == 0 && (((uintptr_t)src | (uintptr_t)out) & 3) == 0)
        hipLaunchKernelGGL(k_guided_apply<1>, grid, dim3(256), 0, st, abar, bbar, src, out, h, w, Hc, Wc, sx, sy);
    else
        hipLaunchKernelGGL(k_guided_apply<0>, grid, dim3(256), 0, st, abar, bbar, src, out, h, w, Hc, Wc, sx, sy);
    TCL_LAUNCH_RET();
}

}  // extern "C"
