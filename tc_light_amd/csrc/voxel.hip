// Spatio-temporal "Unique Video Tensor" producer on gfx950: the geometry-aware half of the reference's voxelization.
//   SceneFlowDataParser.rgbd2pcd      utils/dataparsers/sceneflow_dataparsers.py:257-274   -> tcl_unproject_sceneflow
//   voxelization(voxel_size != None)  utils/general_utils.py:223-256                       -> tcl_track_mean_f32, tcl_voxel_keys, tcl_unique_rows_i32
// torch.unique(dim=0) is replaced by an open-addressing table of ROW INDICES (linear probing, capacity the next power of two >= 2n): an empty slot
// is claimed with a 32-bit atomicCAS of the row index, an occupied slot is compared through the occupant's key row, equal rows atomicMin their own
// index into the slot.  A claimed slot never changes its key class, so all rows of a class end in one slot and that slot ends holding the class's
// smallest row index whatever the race order: ids are numbered by first appearance in row order and are bit-identical from run to run (the
// reference numbers by lexicographic rank -- a permutation of codebook rows; the partition is the same).  The ranks come from a three-launch
// exclusive scan of the representative flags (tile counts, one block over the tile counts, tile-local scan + offset): no spinning, no atomics.
#include "common.h"
#include "../../include/tclight_hip.h"

#define VOX_EMPTY_BYTE 0x7F                            // hipMemset pattern: every slot = 0x7F7F7F7F, above any row index (n <= 2^30)
#define VOX_EMPTY 0x7F7F7F7F
#define VOX_TILE 1024                                  // scan tile: 256 threads x 4 rows

// ----------------------------------------------------------------------------------------------------------------- unprojection
__global__ void k_unproject(const float* __restrict__ depth, const float* __restrict__ c2w, int P, int W, float fx, float fy, float cx, float cy,
                            float* __restrict__ out) {
#pragma clang fp contract(off)
    const int n = blockIdx.y;
    const float* M = c2w + (size_t)n * 16;
    float m[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) m[j] = M[j];
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const int py = p / W, px = p - py * W;
        const float d = depth[(size_t)n * P + p];
        const float x = ((float)px - cx) * d / fx;         // product then quotient (sceneflow_dataparsers.py:267-268)
        const float y = ((float)py - cy) * d / fy;
        const float ny = -y, nd = -d;                      // (x, -y, -d, 1) @ c2w^T, first three components (:270-271)
        float* o = out + (size_t)n * 3 * P + p;
#pragma unroll
        for (int j = 0; j < 3; ++j) o[(size_t)j * P] = ((x * m[4 * j] + ny * m[4 * j + 1]) + nd * m[4 * j + 2]) + m[4 * j + 3];
    }
}

// ----------------------------------------------------------------------------------------------------------------- per-track means
// one frame per launch: ids are distinct inside a frame, so the read-modify-write below has no conflict, and a track's sum takes its addends in
// frame order -- what a sequential CPU scatter in row order computes.
__global__ void k_track_accum(const float* __restrict__ val, const int* __restrict__ ids, float* __restrict__ sum, float* __restrict__ cnt,
                              int P, int C, size_t K) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const int id = ids[p];
        if (id < 0 || (size_t)id >= K) continue;          // never write outside [K,C]
        for (int c = 0; c < C; ++c) sum[(size_t)id * C + c] += val[(size_t)c * P + p];
        cnt[id] += 1.f;
    }
}
__global__ void k_track_final(float* __restrict__ mean, const float* __restrict__ cnt, int C, size_t K) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < K * C; i += (size_t)gridDim.x * blockDim.x)
        mean[i] = mean[i] / fmaxf(cnt[i / C], 1.f);      // torch_scatter 'mean': sum / clamp(count, 1)
}

// ----------------------------------------------------------------------------------------------------------------- voxel keys
// c10::div_floor_floating (torch's div(rounding_mode='floor') on floats): fmod, subtract, divide, sign fix, floor with its 0.5 correction.
__device__ __forceinline__ float floor_div(float a, float b) {
#pragma clang fp contract(off)
    if (b == 0.f) return a / b;
    const float mod = fmodf(a, b);
    float div = (a - mod) / b;
    if (mod != 0.f && (b < 0.f) != (mod < 0.f)) div -= 1.f;
    float fd;
    if (div != 0.f) {
        fd = floorf(div);
        if (div - fd > 0.5f) fd += 1.f;
    } else {
        fd = copysignf(0.f, a / b);
    }
    return fd;
}
__device__ __forceinline__ int key_i32(float f) {        // saturating; NaN -> 0
    if (!(f == f)) return 0;
    if (f >= 2147483648.f) return 0x7FFFFFFF;
    if (f <= -2147483648.f) return (int)0x80000000;
    return (int)f;
}
__global__ void k_voxel_keys(const float* __restrict__ rgb, const float* __restrict__ xyz, const float* __restrict__ xyz_min, float voxel,
                             float rgb_voxel, size_t K, int* __restrict__ keys) {
#pragma clang fp contract(off)
    const float mn[3] = {xyz_min[0], xyz_min[1], xyz_min[2]};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < K; i += (size_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            keys[i * 6 + c] = key_i32(floor_div(xyz[i * 3 + c] - mn[c], voxel));
            keys[i * 6 + 3 + c] = key_i32(floor_div(rgb[i * 3 + c], rgb_voxel));
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- unique rows
__device__ __forceinline__ unsigned mix32(unsigned h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__global__ void k_rows_insert(const int* __restrict__ keys, size_t n, int C, int* __restrict__ table, unsigned mask, int* __restrict__ slot) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        int k[6];
        unsigned h = 0x9E3779B9u;
        for (int c = 0; c < C; ++c) { k[c] = keys[i * C + c]; h = mix32(h ^ (unsigned)k[c]) + 0x9E3779B9u * (unsigned)(c + 1); }
        h &= mask;
        // terminates: the table has at least n free slots more than rows, so a probe run always meets an empty slot or the row's own class
        for (;;) {
            const int old = atomicCAS(table + h, VOX_EMPTY, (int)i);
            if (old == VOX_EMPTY) break;                                         // claimed: this slot is now the class's
            bool eq = true;
            for (int c = 0; c < C; ++c) eq = eq && keys[(size_t)old * C + c] == k[c];
            if (eq) { if ((int)i < old) atomicMin(table + h, (int)i); break; }   // same class: keep the smallest row index
            h = (h + 1u) & mask;
        }
        slot[i] = (int)h;                              // h < 2^31: stored as its bit pattern
    }
}
// flag(i) = 1 when row i is its class's representative (its slot holds i)
__device__ __forceinline__ int rep_flag(const int* table, const int* slot, size_t i) { return table[(unsigned)slot[i]] == (int)i; }

__global__ __launch_bounds__(256) void k_rows_tile_count(const int* __restrict__ table, const int* __restrict__ slot, size_t n, int* __restrict__ tsum) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x;
    const size_t p0 = (size_t)blockIdx.x * VOX_TILE + (size_t)tid * 4;
    int loc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (p0 + j < n) loc += rep_flag(table, slot, p0 + j);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) loc += __shfl_xor(loc, o, 64);
    if ((tid & 63) == 0) s_w[tid >> 6] = loc;
    __syncthreads();
    if (tid == 0) tsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
// one block: tsum[t] <- exclusive prefix, *count <- total.  nt <= 2^20.
__global__ __launch_bounds__(1024) void k_rows_tile_scan(int* __restrict__ tsum, int nt, int* __restrict__ count) {
    __shared__ int s_w[16], s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < nt; base += 1024) {
        const int t = base + tid;
        const int v = t < nt ? tsum[t] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        int woff = 0, total = 0;
        for (int j = 0; j < 16; ++j) { if (j < wv) woff += s_w[j]; total += s_w[j]; }
        const int carry = s_carry;
        if (t < nt) tsum[t] = carry + woff + incl - v;
        __syncthreads();
        if (tid == 0) s_carry = carry + total;
        __syncthreads();
    }
    if (tid == 0) *count = s_carry;
}
__global__ __launch_bounds__(256) void k_rows_rank(const int* __restrict__ table, const int* __restrict__ slot, size_t n, const int* __restrict__ tsum,
                                                   int* __restrict__ rank) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t p0 = (size_t)blockIdx.x * VOX_TILE + (size_t)tid * 4;
    int f[4], loc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = p0 + j < n ? rep_flag(table, slot, p0 + j) : 0; loc += f[j]; }
    int incl = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int off = tsum[blockIdx.x] + incl - loc;
    for (int j = 0; j < wv; ++j) off += s_w[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) if (p0 + j < n) { rank[p0 + j] = off; off += f[j]; }
}
// inv[i] = rank[representative of i]; `inv` holds the slots on entry (each thread reads its own entry before it writes it)
__global__ void k_rows_inverse(const int* __restrict__ table, const int* __restrict__ rank, size_t n, int* inv) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        inv[i] = rank[table[(unsigned)inv[i]]];
}

static inline size_t rows_capacity(size_t n) { size_t c = 2; while (c < 2 * n) c <<= 1; return c; }
static inline size_t rows_tiles(size_t n) { return (n + VOX_TILE - 1) / VOX_TILE; }

extern "C" {

int tcl_unproject_sceneflow(const float* depth, const float* c2w, int N, int H, int W, float fx, float fy, float cx, float cy, float* p_world,
                            hipStream_t st) {
    TCL_CHECK_ARG(depth && c2w && p_world && N > 0 && N <= 65535 && H > 0 && W > 0 && (size_t)H * W < 0x7FFFFFFFull && fx != 0.f && fy != 0.f);
    const int P = H * W;
    int g = stream_grid(P, 256, 2); if (g > 2048) g = 2048;
    hipLaunchKernelGGL(k_unproject, dim3(g, N), dim3(256), 0, st, depth, c2w, P, W, fx, fy, cx, cy, p_world);
    TCL_LAUNCH_RET();
}

int tcl_track_mean_f32(const float* values, const int* ids, int N, int C, int H, int W, size_t K, float* mean, float* cnt, hipStream_t st) {
    TCL_CHECK_ARG(values && ids && mean && cnt && N > 0 && C >= 1 && C <= 3 && H > 0 && W > 0 && (size_t)H * W < 0x7FFFFFFFull && K > 0 &&
                  K <= 0x7FFFFFFFull);
    const int P = H * W;
    if (hipMemsetAsync(mean, 0, K * C * 4, st) != hipSuccess || hipMemsetAsync(cnt, 0, K * 4, st) != hipSuccess) return TCL_ELAUNCH;
    int g = stream_grid(P, 256, 2); if (g > 2048) g = 2048;
    for (int f = 0; f < N; ++f)
        hipLaunchKernelGGL(k_track_accum, dim3(g), dim3(256), 0, st, values + (size_t)f * C * P, ids + (size_t)f * P, mean, cnt, P, C, K);
    hipLaunchKernelGGL(k_track_final, dim3(stream_grid((long)(K * C), 256, 4)), dim3(256), 0, st, mean, cnt, C, K);
    TCL_LAUNCH_RET();
}

int tcl_voxel_keys(const float* mean_rgb, const float* mean_xyz, const float* xyz_min, float voxel_size, float rgb_vox_size, size_t K, int* keys,
                   hipStream_t st) {
    TCL_CHECK_ARG(mean_rgb && mean_xyz && xyz_min && keys && K > 0 && K <= 0x7FFFFFFFull);
    hipLaunchKernelGGL(k_voxel_keys, dim3(stream_grid((long)K, 256, 1)), dim3(256), 0, st, mean_rgb, mean_xyz, xyz_min, voxel_size, rgb_vox_size, K,
                       keys);
    TCL_LAUNCH_RET();
}

size_t tcl_unique_rows_workspace_bytes(size_t n) {
    if (n == 0 || n > (1ull << 30)) return 0;
    return rows_capacity(n) * 4 + n * 4 + (rows_tiles(n) + 1) * 4 + 256;       // table | rank | tile sums
}
int tcl_unique_rows_i32(const int* keys, size_t n, int C, int* inv, int* count, void* ws, hipStream_t st) {
    TCL_CHECK_ARG(keys && inv && count && ws && n >= 1 && n <= (1ull << 30) && C >= 1 && C <= 6);
    const size_t cap = rows_capacity(n), nt = rows_tiles(n);
    int* table = (int*)ws;
    int* rank = table + cap;
    int* tsum = rank + n;
    if (hipMemsetAsync(table, VOX_EMPTY_BYTE, cap * 4, st) != hipSuccess) return TCL_ELAUNCH;      // the call clears its own table
    const int g = stream_grid((long)n, 256, 1);
    hipLaunchKernelGGL(k_rows_insert, dim3(g), dim3(256), 0, st, keys, n, C, table, (unsigned)(cap - 1), inv);
    hipLaunchKernelGGL(k_rows_tile_count, dim3((unsigned)nt), dim3(256), 0, st, table, inv, n, tsum);
    hipLaunchKernelGGL(k_rows_tile_scan, dim3(1), dim3(1024), 0, st, tsum, (int)nt, count);
    hipLaunchKernelGGL(k_rows_rank, dim3((unsigned)nt), dim3(256), 0, st, table, inv, n, tsum, rank);
    hipLaunchKernelGGL(k_rows_inverse, dim3(g), dim3(256), 0, st, table, rank, n, inv);
    TCL_LAUNCH_RET();
}

}  // extern "C"
