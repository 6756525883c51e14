// generation.keyframes: only every K-th frame (the keys) is denoised; the frames in between are the source frame times the gain field relit / source
// of their two neighbouring keys, carried along the chained optical flows and blended by distance.  The arithmetic is spelled out at the prototypes in
// include/tclight_hip.h; the tests restate it in float64 from there.
//   k_flow_chain          one launch per distance d from the key: thread = pixel of one (frame, direction).  Round trip 1: the frame's own flow at p.
//                         Round trip 2: the 4 taps x 2 components of the neighbour's opposite flow (the forward-backward check) and, for d > 1, the
//                         4 taps x 3 planes of the chain of distance d-1 -- 20 independent loads, all issued before the first is used (the addresses
//                         are clamped into the frame, so no load sits behind a guard).
//   k_keyframe_propagate  thread = pixel of one frame.  Round trip 1: S_i(p), CL[i](p), CR[i](p) (9 loads).  Round trip 2: 4 taps x 3 channels of the
//                         source and the relit frame of both keys (48 loads).  A hole (visible in neither key; rare, and whole regions at once) reads the
//                         two keys at p itself in a third trip.  Key frames are copied.
// HBM traffic per pixel: chain 40 B per (frame, direction, distance): 8 own flow + 8 opposite flow + 12 previous chain + 12 out; propagate 96 B per
// non-key frame: 12 S_i + 24 chains + 48 the two keys' source and relit frames (every tap is its neighbours' tap too: L2 hits) + 12 out.
// The per-frame tables travel as kernel arguments (a batch is at most 33 frames): a block's table reads are scalar loads of the kernarg segment.
#include <math.h>
#include "common.h"
#include "../../include/tclight_hip.h"

#pragma clang fp contract(off)

// KEEP(x) pins a loaded value at its place in the program: hipcc otherwise orders a pixel's loads by their uses (one key's taps after the other's
// arithmetic) -- the loads of a thread then run one round trip after the other.
#define KEEP(x) asm volatile("" :: "v"(x))

namespace {

constexpr int TW = TCL_KEYFRAME_TILE_W, TH = TCL_KEYFRAME_TILE_H, SLOTS = TCL_KEYFRAME_BATCH_FRAMES, GAP = TCL_KEYFRAME_MAX_GAP;
static_assert(TW == 64 && TW * TH == 256, "the kernels below are written for 256 lanes: 64 columns x 4 rows");

struct Taps { int o00, o01, o10, o11; float fx, fy; };

// the four tap offsets and the two fractions of bil(., q); q is clamped first, so the offsets are inside the frame whatever q is (NaN -> 0)
__device__ __forceinline__ Taps taps_at(float qx, float qy, int H, int W) {
    qx = fminf(fmaxf(qx, 0.f), (float)(W - 1));
    qy = fminf(fmaxf(qy, 0.f), (float)(H - 1));
    const float x0f = floorf(qx), y0f = floorf(qy);
    const int x0 = (int)x0f, y0 = (int)y0f, x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    return {y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1, qx - x0f, qy - y0f};
}

__device__ __forceinline__ float bil(float t00, float t01, float t10, float t11, float fx, float fy) {
    const float top = t00 + fx * (t01 - t00);
    const float bot = t10 + fx * (t11 - t10);
    return top + fy * (bot - top);
}

__device__ __forceinline__ bool inb(float qx, float qy, int H, int W) {
    return qx >= 0.f && qx <= (float)(W - 1) && qy >= 0.f && qy <= (float)(H - 1);
}

// jobs of one distance: slot[0 .. n_left) are the frames that chain towards their left key, slot[n_left .. n) towards their right key
struct ChainJobs { int n_left, n; unsigned char slot[2 * SLOTS]; };

template <bool FIRST>
__global__ __launch_bounds__(256) void k_flow_chain(const float* __restrict__ fut, const float* __restrict__ past, float* ws, int f0, int H, int W,
                                                    float alpha, ChainJobs jobs) {
    const int x = blockIdx.x * TW + (threadIdx.x & (TW - 1)), y = blockIdx.y * TH + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int job = blockIdx.z, s = jobs.slot[job];
    const bool right = job >= jobs.n_left;
    const long hw = (long)H * W, j = f0 + s;
    const float* A = (right ? fut : past) + j * 2 * hw;                                    // the frame's own flow towards the key
    const float* B = right ? past + (j + 1) * 2 * hw : fut + (j - 1) * 2 * hw;              // the neighbour's flow back
    const float* P = ws + ((long)(right ? s + 1 : s - 1) * 2 + (right ? 1 : 0)) * 3 * hw;   // the neighbour's chain (distance d - 1)
    float* O = ws + ((long)s * 2 + (right ? 1 : 0)) * 3 * hw;
    const int p = y * W + x;
    const float ax = A[p], ay = A[hw + p];
    const float qx = (float)x + ax, qy = (float)y + ay;
    const Taps t = taps_at(qx, qy, H, W);
    const int o[4] = {t.o00, t.o01, t.o10, t.o11};
    float b[2][4], c[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b[0][k] = B[o[k]]; b[1][k] = B[hw + o[k]];
        if (!FIRST) { c[0][k] = P[o[k]]; c[1][k] = P[hw + o[k]]; c[2][k] = P[2 * hw + o[k]]; }
    }
    const float gx = bil(b[0][0], b[0][1], b[0][2], b[0][3], t.fx, t.fy), gy = bil(b[1][0], b[1][1], b[1][2], b[1][3], t.fx, t.fy);
    const float ex = ax + gx, ey = ay + gy;
    const float lhs = ex * ex + ey * ey;
    const float na = sqrtf(ax * ax + ay * ay), ng = sqrtf(gx * gx + gy * gy);
    const float th = alpha * (na + ng) + alpha;
    bool valid = inb(qx, qy, H, W) && lhs < th * th;
    float cx = ax, cy = ay;
    if (!FIRST) {
        cx = ax + bil(c[0][0], c[0][1], c[0][2], c[0][3], t.fx, t.fy);
        cy = ay + bil(c[1][0], c[1][1], c[1][2], c[1][3], t.fx, t.fy);
        valid = valid && c[2][0] == 1.f && c[2][1] == 1.f && c[2][2] == 1.f && c[2][3] == 1.f;
    }
    O[p] = valid ? cx : 0.f;
    O[hw + p] = valid ? cy : 0.f;
    O[2 * hw + p] = valid ? 1.f : 0.f;
}

// per slot of the batch: the frames fa / fb of the two keys (a key frame: both its own), ka the index of the left one among the keys, the weights
struct PropJobs { int fa[SLOTS], fb[SLOTS], ka[SLOTS]; float ta[SLOTS], tb[SLOTS]; };

__global__ __launch_bounds__(256) void k_keyframe_propagate(const float* __restrict__ src, const float* __restrict__ keys,
                                                            const float* __restrict__ ws, float* __restrict__ out, unsigned* __restrict__ holes,
                                                            int f0, int H, int W, float thr, float eps, PropJobs jobs) {
    const int x = blockIdx.x * TW + (threadIdx.x & (TW - 1)), y = blockIdx.y * TH + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int s = blockIdx.z;
    const long hw = (long)H * W, i = f0 + s;
    const int p = y * W + x;
    const long fa = jobs.fa[s], fb = jobs.fb[s], ka = jobs.ka[s];
    float* po = out + i * 3 * hw + p;
    if (fa == i) {                                              // a key frame (the same answer in the whole block): the bits of relit_keys
        const float* pk = keys + ka * 3 * hw + p;
        const float v0 = pk[0], v1 = pk[hw], v2 = pk[2 * hw];
        po[0] = v0; po[hw] = v1; po[2 * hw] = v2;
        return;
    }
    const float ta = jobs.ta[s], tb = jobs.tb[s];
    const float* S[2] = {src + fa * 3 * hw, src + fb * 3 * hw};
    const float* R[2] = {keys + ka * 3 * hw, keys + (ka + 1) * 3 * hw};
    const float* pc = ws + (long)s * 6 * hw + p;
    const float* pi = src + i * 3 * hw + p;
    float si[3], ch[2][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { si[c] = pi[c * hw]; ch[0][c] = pc[c * hw]; ch[1][c] = pc[(3 + c) * hw]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) { KEEP(si[c]); KEEP(ch[0][c]); KEEP(ch[1][c]); }
    Taps t[2];
    float sv[2][3][4], rv[2][3][4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        t[k] = taps_at((float)x + ch[k][0], (float)y + ch[k][1], H, W);
        const int o[4] = {t[k].o00, t[k].o01, t[k].o10, t[k].o11};
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int n = 0; n < 4; ++n) { sv[k][c][n] = S[k][c * hw + o[n]]; rv[k][c][n] = R[k][c * hw + o[n]]; }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int n = 0; n < 4; ++n) { KEEP(sv[k][c][n]); KEEP(rv[k][c][n]); }
    float w[2], G[2][3];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float m = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float sc = bil(sv[k][c][0], sv[k][c][1], sv[k][c][2], sv[k][c][3], t[k].fx, t[k].fy);
            const float rc = bil(rv[k][c][0], rv[k][c][1], rv[k][c][2], rv[k][c][3], t[k].fx, t[k].fy);
            m = fmaxf(m, fabsf(sc - si[c]));
            G[k][c] = (rc + eps) / (sc + eps);
        }
        w[k] = (k == 0 ? ta : tb) * ch[k][2] * (m < thr ? 1.f : 0.f);
    }
    const float wsum = w[0] + w[1];
    float g[3];
    if (wsum > 0.f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = (w[0] * G[0][c] + w[1] * G[1][c]) / wsum;
    } else {
        float ga[3], gb[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ga[c] = (R[0][c * hw + p] + eps) / (S[0][c * hw + p] + eps);
            gb[c] = (R[1][c * hw + p] + eps) / (S[1][c * hw + p] + eps);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = ta * ga[c] + tb * gb[c];
        atomicAdd(&holes[i], 1u);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) po[c * hw] = (si[c] + eps) * g[c] - eps;
}

bool keys_ok(const int* k, int M, int N) {
    if (M < 1 || k[0] != 0 || k[M - 1] != N - 1) return false;
    for (int g = 0; g + 1 < M; ++g)
        if (k[g + 1] <= k[g] || k[g + 1] - k[g] > GAP) return false;
    return true;
}

bool positive(float v) { return v > 0.f && v < INFINITY; }      // NaN fails

// what both entries check alike; -> the batch's first frame and its number of frames
int check_batch(const int* h_keys, int M, int g0, int g1, int N, int H, int W, const void* ws, long ws_bytes, int* f0, int* span) {
    TCL_CHECK_ARG(h_keys && ws && N > 0 && H > 0 && W > 0 && M > 0 && M <= N);
    TCL_CHECK_ARG((long)H * W <= (1L << 30) && cdiv(H, TH) <= 65535);
    TCL_CHECK_ARG(keys_ok(h_keys, M, N));
    TCL_CHECK_ARG(g0 >= 0 && g0 <= g1 && g1 <= M - 1);
    *f0 = h_keys[g0];
    *span = h_keys[g1] - h_keys[g0] + 1;
    TCL_CHECK_ARG(*span <= SLOTS);
    TCL_CHECK_ARG(ws_bytes >= 0 && (size_t)ws_bytes >= (size_t)*span * 6 * H * W * sizeof(float) && ((uintptr_t)ws & 3) == 0);
    return TCL_OK;
}

}  // namespace

extern "C" {

size_t tcl_keyframe_workspace_bytes(int N, int H, int W, int K) {
    if (N <= 0 || H <= 0 || W <= 0 || K < 1 || K > GAP || (long)H * W > (1L << 30)) return 0;
    return (size_t)(N < SLOTS ? N : SLOTS) * 6 * H * W * sizeof(float);
}

int tcl_flow_chain_f32(const float* fut, const float* past, const int* h_keys, int M, int g0, int g1, int N, int H, int W, float alpha, void* ws,
                       long ws_bytes, hipStream_t st) {
    TCL_CHECK_ARG(fut && past && positive(alpha));
    int f0, span;
    if (int r = check_batch(h_keys, M, g0, g1, N, H, W, ws, ws_bytes, &f0, &span)) return r;
    for (int d = 1; d < GAP; ++d) {
        ChainJobs jobs = {};
        int right[SLOTS], nr = 0;
        for (int g = g0; g < g1; ++g)
            if (h_keys[g + 1] - h_keys[g] > d) {
                jobs.slot[jobs.n_left++] = (unsigned char)(h_keys[g] + d - f0);
                right[nr++] = h_keys[g + 1] - d - f0;
            }
        if (jobs.n_left == 0) break;
        for (int k = 0; k < nr; ++k) jobs.slot[jobs.n_left + k] = (unsigned char)right[k];
        jobs.n = jobs.n_left + nr;
        const dim3 grid(cdiv(W, TW), cdiv(H, TH), jobs.n);
        if (d == 1)
            hipLaunchKernelGGL(k_flow_chain<true>, grid, dim3(256), 0, st, fut, past, (float*)ws, f0, H, W, alpha, jobs);
        else
            hipLaunchKernelGGL(k_flow_chain<false>, grid, dim3(256), 0, st, fut, past, (float*)ws, f0, H, W, alpha, jobs);
    }
    TCL_LAUNCH_RET();
}

int tcl_keyframe_propagate_f32(const float* source, const float* relit_keys, float* out, unsigned* holes, const int* h_keys, int M, int g0, int g1,
                               const int* h_left, const int* h_right, const float* h_tw, int N, int H, int W, float diff_threshold, float eps,
                               const void* ws, long ws_bytes, hipStream_t st) {
    TCL_CHECK_ARG(source && relit_keys && out && holes && h_left && h_right && h_tw && positive(diff_threshold) && eps > 0.f && eps <= 0.25f);
    int f0, span;
    if (int r = check_batch(h_keys, M, g0, g1, N, H, W, ws, ws_bytes, &f0, &span)) return r;
    for (int i = 0, g = 0; i < N; ++i) {                         // the tables of ALL frames agree with the keys
        if (g + 1 < M && h_keys[g + 1] <= i) ++g;                // g: the last key at or before i
        TCL_CHECK_ARG(h_left[i] == g && h_right[i] == (h_keys[g] == i ? g : g + 1));
        TCL_CHECK_ARG(h_tw[i] >= 0.f && h_tw[i] <= 1.f && h_tw[N + i] >= 0.f && h_tw[N + i] <= 1.f);
    }
    PropJobs jobs = {};
    for (int s = 0; s < span; ++s) {
        const int i = f0 + s;
        jobs.fa[s] = h_keys[h_left[i]]; jobs.fb[s] = h_keys[h_right[i]]; jobs.ka[s] = h_left[i];
        jobs.ta[s] = h_tw[i]; jobs.tb[s] = h_tw[N + i];
    }
    if (hipMemsetAsync(holes + f0, 0, (size_t)span * sizeof(unsigned), st) != hipSuccess) return TCL_ELAUNCH;
    hipLaunchKernelGGL(k_keyframe_propagate, dim3(cdiv(W, TW), cdiv(H, TH), span), dim3(256), 0, st, source, relit_keys, (const float*)ws, out, holes,
                       f0, H, W, diff_threshold, eps, jobs);
    TCL_LAUNCH_RET();
}

}  // extern "C"
