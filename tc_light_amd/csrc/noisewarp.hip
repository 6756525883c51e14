// generation.noise_mode warp: the noise of a clip is a field F_t [4,H,W] at PIXEL resolution that is carried from frame to frame along the backward optical
// flow and stays white and unit-variance in every frame; the latent noise of a frame is the normalised 8 x 8 block sum of its field.  The arithmetic is
// spelled out at the prototypes in include/tclight_hip.h; tests/noisewarp_refs.py restates it in numpy from there.
//   k_noise_count   thread = pixel (64 x 4 tiles).  One round trip: flow (2), mask, G_t (4) -- 7 independent loads.  A valid pixel then adds 1 to k and
//                   llrintf(G * 2^24) to the four 64-bit sums of its source q: integer atomics, so the result does not depend on the order of arrival.
//   k_noise_apply   block = 64 x 8 pixels = 8 latent columns x 1 latent row, 256 threads x 2 pixels (rows r and r + 4).  Round trip 1: flow, mask, G_t of
//                   both pixels (14 loads).  Round trip 2: k[q] and F_{t-1}[q] (4 channels) of both pixels (10 loads; q is replaced by p itself where
//                   the pixel is invalid, so no load sits behind a guard).  Only a pixel with k > 1 reads its four sums in a third trip: the plain copy
//                   pays for k alone.  F_t goes to memory and into an LDS tile, from which the 8 x 8 sums are taken in the fixed order of the header.
//                   FIRST (t = 0): F_0 = G_0, no flow, mask, k or F_{t-1} is read.
// HBM traffic per pixel and frame: clear 36 B, count 28 B read + 36 B of atomics where valid, apply 28 + 20 read (+ 32 where k > 1) + 16 written: ~150 B.
#include <math.h>
#include "common.h"
#include "../../include/tclight_hip.h"

#pragma clang fp contract(off)

// KEEP(x) pins a loaded value at its place in the program, so that the loads of one round trip are all issued before the first is used
#define KEEP(x) asm volatile("" :: "v"(x))

namespace {

constexpr int TW = TCL_NOISE_WARP_TILE_W, CELL = TCL_NOISE_WARP_CELL;
static_assert(TW == 64 && CELL == 8, "the kernels below are written for 64 x 8 pixel tiles of 8 x 8 cells");
constexpr int ROW = TW + TW / CELL;                     // LDS row of the tile: column c sits at c + c / 8, so the 8 cells of a row start in 8 banks

// the source of pixel (x, y): q = (rintf(x + u), rintf(y + v)), nearest-even; -> its offset in the plane, or -1 where p is invalid (q outside the frame,
// a NaN / inf flow, or a mask that is not > 0.5: every comparison with a NaN is false)
__device__ __forceinline__ int source_of(int x, int y, float u, float v, float m, int H, int W) {
    const float qx = rintf((float)x + u), qy = rintf((float)y + v);
    const bool valid = qx >= 0.f && qx <= (float)(W - 1) && qy >= 0.f && qy <= (float)(H - 1) && m > 0.5f;
    return valid ? (int)qy * W + (int)qx : -1;
}

__global__ __launch_bounds__(256) void k_noise_count(const float* __restrict__ flow, const float* __restrict__ mask, const float* __restrict__ G,
                                                     unsigned long long* __restrict__ sums, int* __restrict__ cnt, int H, int W) {
    const int x = blockIdx.x * TW + (threadIdx.x & (TW - 1)), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t hw = (size_t)H * W;
    const int p = y * W + x;
    const float u = flow[p], v = flow[hw + p], m = mask[p];
    float g[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) g[c] = G[c * hw + p];
    const int q = source_of(x, y, u, v, m, H, W);
    if (q < 0) return;
    atomicAdd(&cnt[q], 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) atomicAdd(&sums[c * hw + q], (unsigned long long)llrintf(g[c] * 16777216.f));      // two's complement: the sum is signed
}

template <bool FIRST>
__global__ __launch_bounds__(256) void k_noise_apply(const float* __restrict__ flow, const float* __restrict__ mask, const float* __restrict__ G,
                                                     const float* __restrict__ Fp, const long long* __restrict__ sums, const int* __restrict__ cnt,
                                                     float* __restrict__ F, float* __restrict__ z, int H, int W) {
    __shared__ float tile[4][CELL][ROW];
    __shared__ float rows[4][CELL][TW / CELL];
    const int tx = threadIdx.x & (TW - 1), ty = threadIdx.x >> 6;
    const int x = blockIdx.x * TW + tx;
    const size_t hw = (size_t)H * W;
    if (x < W) {                                            // H is a multiple of 8: the tile's 8 rows are all inside
        int p[2], q[2] = {-1, -1}, k[2] = {0, 0};
        float u[2], v[2], m[2], g[2][4], f[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            p[j] = (blockIdx.y * CELL + ty + 4 * j) * W + x;
            if (!FIRST) { u[j] = flow[p[j]]; v[j] = flow[hw + p[j]]; m[j] = mask[p[j]]; }
#pragma unroll
            for (int c = 0; c < 4; ++c) g[j][c] = G[c * hw + p[j]];
        }
        if (!FIRST) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                KEEP(u[j]); KEEP(v[j]); KEEP(m[j]);
#pragma unroll
                for (int c = 0; c < 4; ++c) KEEP(g[j][c]);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                q[j] = source_of(x, blockIdx.y * CELL + ty + 4 * j, u[j], v[j], m[j], H, W);
                const int a = q[j] < 0 ? p[j] : q[j];       // an address inside the frame whatever the flow is
                k[j] = cnt[a];
#pragma unroll
                for (int c = 0; c < 4; ++c) f[j][c] = Fp[c * hw + a];
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                KEEP(k[j]);
#pragma unroll
                for (int c = 0; c < 4; ++c) KEEP(f[j][c]);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float o[4];
            if (FIRST || q[j] < 0) {
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = g[j][c];
            } else if (k[j] <= 1) {                         // k == 1 (k is at least 1 at the source of a valid pixel): the copy, bit for bit
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = f[j][c];
            } else {
                long long s[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) s[c] = sums[c * hw + q[j]];
                const float root = sqrtf((float)k[j]);
                const double den = 16777216.0 * (double)k[j];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float mean = (float)((double)s[c] / den);
                    const float a = f[j][c] / root, b = g[j][c] - mean;
                    o[c] = a + b;
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                F[c * hw + p[j]] = o[c];
                tile[c][ty + 4 * j][tx + tx / CELL] = o[c];
            }
        }
    }
    __syncthreads();
    {   // the 8 pixels of one row of one cell, left to right
        const int c = threadIdx.x >> 6, r = (threadIdx.x >> 3) & 7, cell = threadIdx.x & 7;
        if (blockIdx.x * TW + cell * CELL < W) {
            const float* t = &tile[c][r][cell * (CELL + 1)];
            float s = t[0];
#pragma unroll
            for (int i = 1; i < CELL; ++i) s = s + t[i];
            rows[c][r][cell] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 * (TW / CELL)) {                    // the 8 row sums of one cell, top to bottom, then one multiplication by 1/8
        const int c = threadIdx.x >> 3, cell = threadIdx.x & 7;
        const int lx = blockIdx.x * (TW / CELL) + cell, w = W / CELL, h = H / CELL;
        if (lx < w) {
            float s = rows[c][0][cell];
#pragma unroll
            for (int r = 1; r < CELL; ++r) s = s + rows[c][r][cell];
            z[((size_t)c * h + blockIdx.y) * w + lx] = s * 0.125f;
        }
    }
}

bool size_ok(int H, int W) {
    return H > 0 && W > 0 && H % CELL == 0 && W % CELL == 0 && (long)H * W <= (1L << 30) && H <= 4 * 65535;
}

}  // namespace

extern "C" {

size_t tcl_noise_warp_workspace_bytes(int H, int W) {
    if (!size_ok(H, W)) return 0;
    return (size_t)H * W * (4 * sizeof(long long) + sizeof(int));
}

int tcl_noise_warp_count(const float* past_flows, const float* mask_bwds, const float* G, int t, int N, int H, int W, void* ws, long ws_bytes,
                         hipStream_t st) {
    TCL_CHECK_ARG(past_flows && mask_bwds && G && ws && size_ok(H, W) && N > 0 && t >= 1 && t < N);
    const size_t hw = (size_t)H * W, need = tcl_noise_warp_workspace_bytes(H, W);
    TCL_CHECK_ARG(ws_bytes >= 0 && (size_t)ws_bytes >= need && ((uintptr_t)ws & 7) == 0);
    if (hipMemsetAsync(ws, 0, need, st) != hipSuccess) return TCL_ELAUNCH;
    unsigned long long* sums = (unsigned long long*)ws;
    hipLaunchKernelGGL(k_noise_count, dim3(cdiv(W, TW), cdiv(H, 4)), dim3(256), 0, st, past_flows + (size_t)t * 2 * hw, mask_bwds + (size_t)t * hw, G,
                       sums, (int*)(sums + 4 * hw), H, W);
    TCL_LAUNCH_RET();
}

int tcl_noise_warp_apply_f32(const float* past_flows, const float* mask_bwds, const float* G, const float* F_prev, float* F, float* z, int t, int N,
                             int H, int W, const void* ws, long ws_bytes, hipStream_t st) {
    TCL_CHECK_ARG(G && F && z && size_ok(H, W) && N > 0 && t >= 0 && t < N && G != F);
    const size_t hw = (size_t)H * W;
    float* zt = z + (size_t)t * 4 * (hw / (CELL * CELL));
    const dim3 grid(cdiv(W, TW), H / CELL);
    if (t == 0) {
        hipLaunchKernelGGL(k_noise_apply<true>, grid, dim3(256), 0, st, nullptr, nullptr, G, nullptr, nullptr, nullptr, F, zt, H, W);
        TCL_LAUNCH_RET();
    }
    TCL_CHECK_ARG(past_flows && mask_bwds && F_prev && ws && F_prev != F && F_prev != G);
    TCL_CHECK_ARG(ws_bytes >= 0 && (size_t)ws_bytes >= tcl_noise_warp_workspace_bytes(H, W) && ((uintptr_t)ws & 7) == 0);
    const long long* sums = (const long long*)ws;
    hipLaunchKernelGGL(k_noise_apply<false>, grid, dim3(256), 0, st, past_flows + (size_t)t * 2 * hw, mask_bwds + (size_t)t * hw, G, F_prev, sums,
                       (const int*)(sums + 4 * hw), F, zt, H, W);
    TCL_LAUNCH_RET();
}

}  // extern "C"
