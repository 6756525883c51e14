// OpenAI CLIP (ViT image tower + causal text tower) for the clip-frame / clip-text figures of evaluate.py (evaluate.py:119 clip.load("ViT-B/32");
// utils/evaluation/eval_utils.py:129-161 clip_text / clip_frame).  The Linears and LayerNorms of the towers are tcl_gemm_f16 / tcl_layernorm_f16; this
// file holds what they do not cover.  pick-score (evaluate.py:52-56,120-121; eval_utils.py:163-176 pick_score_func) runs PickScore_v1, a CLIP ViT-H/14, on
// the same kernels: its processor's crop rule and the padded patch rows are options of the preprocess, k_pick_* are its scores.
//
// k_clip_preprocess (one block per 32 x 32 tile of the cropped output of one frame): clip's _transform(n_px) = Resize(n_px, BICUBIC) on a PIL image,
//   CenterCrop, ToTensor, Normalize.  PIL's resampler is integer arithmetic (Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
//   ImagingResampleHorizontal_8bpc / Vertical_8bpc): per output index the bicubic (a = -0.5) weights over a support widened by the down-scale factor
//   are computed in f64, normalised, and rounded to 22-bit fixed point; the horizontal pass is rounded and clipped to uint8 before the vertical pass
//   reads it.  The block computes the coefficient rows of its 32 output columns and 32 output rows (f64, no fma contraction: the operations PIL
//   makes), resamples the input rows its vertical taps touch horizontally into LDS (uint8), and takes the vertical pass from there: only the cropped
//   window is computed and every input byte is read about once.  Outputs: the uint8 crop and / or the normalised f16 patch rows in the column order
//   of conv1.weight.reshape(width, 3 * P * P), so the patch embedding is a plain GEMM.  The rows may be padded to a stride ldp >= 3 P^2 (zeros), for
//   a patch size whose 3 P^2 is not a multiple of the GEMM's K step, and the crop offset follows clip's rounded or transformers' floored rule.
// k_clip_attn<NKP> (one block per (sample, head), 4 waves): reads Q, K, V in place from the fused in_proj output [B*T, 3W].  K ([keys][d], rows
//   padded by 8 halves) and V^T ([d][keys]) of the head sit in LDS, zero-padded to 32 * NKP keys.  A wave takes 16 queries at a time:
//   S^T = K.Q^T with mfma_f32_16x16x32_f16 (lane l: query l & 15, keys 16 t + 4 (l >> 4) + r in accumulator t, register r), so the softmax of a query
//   is in-lane plus two cross-lane steps (xor 16, 32) and exact over the whole row; the f32 probabilities are rounded to f16 in the registers they
//   are in and serve as the B operand of O^T = V^T.P^T: k-slot (l >> 4, j) of pair s then means key 32 s + 16 (j >> 2) + 4 (l >> 4) + (j & 3), and
//   the V^T operand is read from LDS in that same order (two 8-byte reads).  The row sum divides the f32 output.
// k_clip_embed (one block per row): [class | patches] + positional embedding then ln_pre, or token gather + positional embedding; f32 up to the
//   single f16 rounding.   k_quick_gelu: x * sigmoid(1.702 x).
// k_scores_*: cosine statistics of the features in f64 with a fixed summation order (no atomics): repeated runs are bit-identical.
// k_pick_*: PickScore, exp(logit_scale) cos(text, image) per image and the mean, the same way.
#include "common.h"
#include "../../include/tclight_hip.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------ preprocess
constexpr int PT = 32;                  // output tile side
constexpr int PBITS = 32 - 8 - 2;       // PIL's PRECISION_BITS

struct Axis { int in, out, off, ksize; double scale, fscale, support; };

inline Axis make_axis(int in, int out, int off) {
    Axis a;
    a.in = in; a.out = out; a.off = off;
    a.scale = (double)in / (double)out;
    a.fscale = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 2.0 * a.fscale;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    return a;
}

__device__ __forceinline__ double pil_bicubic(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// precompute_coeffs + normalize_coeffs_8bpc for output index xx: bounds[0] = first input index, bounds[1] = tap count, kk[0 .. ksize) the fixed-point taps
__device__ void pil_coeffs(const Axis ax, int xx, int* bounds, int* kk) {
#pragma clang fp contract(off)
    const double center = (xx + 0.5) * ax.scale;
    const double ss = 1.0 / ax.fscale;
    int xmin = (int)(center - ax.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + ax.support + 0.5);
    if (xmax > ax.in) xmax = ax.in;
    xmax -= xmin;
    if (xmax > ax.ksize) xmax = ax.ksize;            // never true for PIL's bounds; keeps the LDS row in range whatever the arguments
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += pil_bicubic((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < ax.ksize; ++x) {
        double w = 0.0;
        if (x < xmax) {
            w = pil_bicubic((x + xmin - center + 0.5) * ss);
            if (ww != 0.0) w /= ww;
        }
        kk[x] = w < 0 ? (int)(-0.5 + w * (1 << PBITS)) : (int)(0.5 + w * (1 << PBITS));
    }
    bounds[0] = xmin; bounds[1] = xmax;
}

__device__ __forceinline__ int clip8(int v) { return min(max(v >> PBITS, 0), 255); }

__global__ __launch_bounds__(256) void k_clip_preprocess(const uint8_t* __restrict__ frames, uint8_t* __restrict__ crop, _Float16* __restrict__ patches,
                                                         int H, int W, int S, int P, int ldp, const Axis ax, const Axis ay, int max_rows) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char smem[];
    int* kx = (int*)smem;                            // [PT][ax.ksize]
    int* ky = kx + PT * ax.ksize;                    // [PT][ay.ksize]
    int* bx = ky + PT * ay.ksize;                    // [PT][2]
    int* by = bx + PT * 2;                           // [PT][2]
    uint8_t* hrow = (uint8_t*)(by + PT * 2);         // [rows][PT][3]: the horizontally resampled input rows of the tile
    const int tid = threadIdx.x, n = blockIdx.z;
    const int ox0 = blockIdx.x * PT, oy0 = blockIdx.y * PT;
    // output indices past the crop are clamped (their results are never stored)
    if (tid < PT) pil_coeffs(ax, ax.off + min(ox0 + tid, S - 1), bx + 2 * tid, kx + tid * ax.ksize);
    else if (tid >= 64 && tid < 64 + PT) pil_coeffs(ay, ay.off + min(oy0 + tid - 64, S - 1), by + 2 * (tid - 64), ky + (tid - 64) * ay.ksize);
    __syncthreads();
    const int y0 = by[0];
    const int rows = min(by[2 * (PT - 1)] + by[2 * (PT - 1) + 1] - y0, max_rows);
    const uint8_t* fr = frames + (long)n * H * W * 3;
    for (int item = tid; item < rows * PT * 3; item += 256) {
        const int r = item / (PT * 3), e = item - r * (PT * 3), col = e / 3, c = e - col * 3;
        const int cnt = bx[2 * col + 1];
        const uint8_t* src = fr + ((long)(y0 + r) * W + bx[2 * col]) * 3 + c;
        const int* k = kx + col * ax.ksize;
        int ss = 1 << (PBITS - 1);
        for (int t = 0; t < cnt; ++t) ss += (int)src[3 * t] * k[t];
        hrow[item] = (uint8_t)clip8(ss);
    }
    __syncthreads();
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    const int npw = S / P;
    for (int item = tid; item < 3 * PT * PT; item += 256) {
        const int c = item / (PT * PT), ty = (item / PT) % PT, tx = item % PT;
        const int oy = oy0 + ty, ox = ox0 + tx;
        const int first = by[2 * ty] - y0, cnt = min(by[2 * ty + 1], rows - first);
        const int* k = ky + ty * ay.ksize;
        int ss = 1 << (PBITS - 1);
        for (int t = 0; t < cnt; ++t) ss += (int)hrow[(first + t) * (PT * 3) + tx * 3 + c] * k[t];
        const int v = clip8(ss);
        if (oy >= S || ox >= S) continue;
        if (crop) crop[(((long)n * S + oy) * S + ox) * 3 + c] = (uint8_t)v;
        if (patches) {
            // ToTensor (uint8 -> f32 / 255) and Normalize ((x - mean) / std), f32, then one rounding to f16
            const float x = ((float)v / 255.f - mean[c]) / stdv[c];
            const long prow = (long)n * npw * npw + (oy / P) * npw + ox / P;
            patches[prow * ldp + (c * P + oy % P) * P + ox % P] = (_Float16)x;
            // the K padding of the row (ldp > 3 P^2: ViT-H/14's 588 -> 640) is zeroed by the thread that holds the patch's first pixel
            if (c == 0 && oy % P == 0 && ox % P == 0)
                for (int j = 3 * P * P; j < ldp; ++j) patches[prow * ldp + j] = (_Float16)0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------ attention
template <int NKP>
__global__ __launch_bounds__(256) void k_clip_attn(const _Float16* __restrict__ qkv, _Float16* __restrict__ out, int T, int H, int d, int DP, float scale,
                                                   int causal) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int TP = 32 * NKP, VS = TP + 8;
    const int KS = DP + 8;
    _Float16* Ks = (_Float16*)smem;                  // [TP][KS]: K rows, columns d .. DP and keys T .. TP zero
    _Float16* Vt = Ks + TP * KS;                     // [d][VS]: V transposed, keys T .. TP zero
    const int tid = threadIdx.x, b = blockIdx.x / H, hh = blockIdx.x % H;
    const int Wd = H * d, ld = 3 * Wd;
    const _Float16* base = qkv + (long)b * T * ld + hh * d;
    const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const int kch = DP / 8, vch = d / 8;
    for (int i = tid; i < TP * kch; i += 256) {
        const int key = i / kch, ch = i - key * kch;
        h8 v = zero8;
        if (key < T && ch * 8 < d) v = *(const h8*)(base + (long)key * ld + Wd + ch * 8);
        *(h8*)(Ks + key * KS + ch * 8) = v;
    }
    for (int i = tid; i < TP * vch; i += 256) {
        const int key = i / vch, ch = i - key * vch;
        h8 v = zero8;
        if (key < T) v = *(const h8*)(base + (long)key * ld + 2 * Wd + ch * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) Vt[(ch * 8 + j) * VS + key] = v[j];
    }
    __syncthreads();
    const int lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int nks = DP / 32, ndt = d / 16;
    for (int qt = tid >> 6; qt * 16 < T; qt += 4) {
        const int q = qt * 16 + c;
        h8 qf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[ks] = zero8;
            if (ks < nks && q < T && 32 * ks + 8 * g < d) qf[ks] = *(const h8*)(base + (long)q * ld + 32 * ks + 8 * g);
        }
        f4 acc[2 * NKP];
#pragma unroll
        for (int t = 0; t < 2 * NKP; ++t) {
            acc[t] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                if (ks < nks) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*(const h8*)(Ks + (16 * t + c) * KS + 32 * ks + 8 * g), qf[ks], acc[t], 0, 0, 0);
        }
        // exact softmax of query q over its keys: in-lane over (t, r), then the 4 lanes that share the query
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2 * NKP; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * t + 4 * g + r;
                const bool ok = key < T && (!causal || key <= q);
                acc[t][r] = ok ? acc[t][r] * scale : -INFINITY;
                m = fmaxf(m, acc[t][r]);
            }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));            // finite: key 0 is never masked
        float sum = 0.f;
        h8 pf[NKP];
#pragma unroll
        for (int t = 0; t < 2 * NKP; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __expf(acc[t][r] - m);
                sum += p;
                pf[t >> 1][(t & 1) * 4 + r] = (_Float16)p;
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;
        for (int dt = 0; dt < ndt; ++dt) {
            f4 o = {0.f, 0.f, 0.f, 0.f};
            const _Float16* vr = Vt + (16 * dt + c) * VS + 4 * g;
#pragma unroll
            for (int s = 0; s < NKP; ++s) {
                const h4 lo = *(const h4*)(vr + 32 * s), hi = *(const h4*)(vr + 32 * s + 16);
                const h8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                o = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[s], o, 0, 0, 0);
            }
            if (q < T) {
                const h4 w = {(_Float16)(o[0] * inv), (_Float16)(o[1] * inv), (_Float16)(o[2] * inv), (_Float16)(o[3] * inv)};
                *(h4*)(out + ((long)b * T + q) * Wd + hh * d + 16 * dt + 4 * g) = w;
            }
        }
    }
}

inline size_t attn_lds(int nkp, int d) {
    const int TP = 32 * nkp, DP = (d + 31) / 32 * 32;
    return ((size_t)TP * (DP + 8) + (size_t)d * (TP + 8)) * 2;
}

template <int NKP>
int launch_attn(const _Float16* qkv, _Float16* out, int B, int T, int H, int d, float scale, int causal, hipStream_t st) {
    const size_t lds = attn_lds(NKP, d);
    if (lds > 160 * 1024) return TCL_EINVAL;
    static bool set = false;
    if (!set) { (void)hipFuncSetAttribute((const void*)k_clip_attn<NKP>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); set = true; }
    hipLaunchKernelGGL(k_clip_attn<NKP>, dim3(B * H), dim3(256), lds, st, qkv, out, T, H, d, (d + 31) / 32 * 32, scale, causal);
    TCL_LAUNCH_RET();
}

// ------------------------------------------------------------------------------------------ embed, QuickGELU
constexpr int EMB_K = 8;                // elements per thread: W <= 2048

__device__ __forceinline__ float block_sum_all(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_clip_embed(const _Float16* __restrict__ patch, const _Float16* __restrict__ cls, const int* __restrict__ ids,
                                                    const _Float16* __restrict__ table, const _Float16* __restrict__ pos, const _Float16* __restrict__ gamma,
                                                    const _Float16* __restrict__ beta, _Float16* __restrict__ out, int T, int W, int vocab, float eps) {
    __shared__ float red[4];
    const long row = blockIdx.x;
    const int t = (int)(row % T);
    const long b = row / T;
    const _Float16* src;
    if (ids) src = table + (long)min(max(ids[row], 0), vocab - 1) * W;          // the binding refuses ids outside the table; the clamp keeps the read in range
    else src = t == 0 ? cls : patch + (b * (T - 1) + t - 1) * W;
    float v[EMB_K];
#pragma unroll
    for (int k = 0; k < EMB_K; ++k) {
        const int i = threadIdx.x + 256 * k;
        v[k] = i < W ? (float)src[i] + (float)pos[(long)t * W + i] : 0.f;
    }
    if (gamma) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < EMB_K; ++k) s += v[k];
        const float mean = block_sum_all(s, red) / W;
        float qv = 0.f;
#pragma unroll
        for (int k = 0; k < EMB_K; ++k) { const float dd = threadIdx.x + 256 * k < W ? v[k] - mean : 0.f; qv += dd * dd; }
        const float rstd = rsqrtf(block_sum_all(qv, red) / W + eps);
#pragma unroll
        for (int k = 0; k < EMB_K; ++k) {
            const int i = threadIdx.x + 256 * k;
            if (i < W) v[k] = (v[k] - mean) * rstd * (float)gamma[i] + (float)beta[i];
        }
    }
#pragma unroll
    for (int k = 0; k < EMB_K; ++k) {
        const int i = threadIdx.x + 256 * k;
        if (i < W) out[row * W + i] = (_Float16)v[k];
    }
}

__global__ __launch_bounds__(256) void k_quick_gelu(const _Float16* __restrict__ x, _Float16* __restrict__ y, long n8) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        const h8 v = *(const h8*)(x + i * 8);
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float f = (float)v[j]; o[j] = (_Float16)(f / (1.f + __expf(-1.702f * f))); }
        *(h8*)(y + i * 8) = o;
    }
}

// ------------------------------------------------------------------------------------------ scores
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_dot(const float* a, const float* b, int D, int lane) {
    double s = 0.0;
    for (int i = lane; i < D; i += 64) s += (double)a[i] * (double)b[i];
    return wave_sum_d(s);
}

// norm[i] = |f_i| for the N feature rows, norm[N] = |text|
__global__ __launch_bounds__(64) void k_scores_norm(const float* __restrict__ f, const float* __restrict__ text, int N, int D, double* __restrict__ norm) {
    const int i = blockIdx.x;
    const float* r = i < N ? f + (long)i * D : text;
    const double s = wave_dot(r, r, D, threadIdx.x);
    if (threadIdx.x == 0) norm[i] = sqrt(s);
}

// part[i] = sum over j != i of cos(f_i, f_j) (wave w takes j = w, w + 4, ...; the four partial sums are joined in wave order); tpart[i] = cos(f_i, text)
__global__ __launch_bounds__(256) void k_scores_row(const float* __restrict__ f, const float* __restrict__ text, int N, int D, const double* __restrict__ norm,
                                                    double* __restrict__ part, double* __restrict__ tpart) {
    __shared__ double red[4];
    const int i = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* fi = f + (long)i * D;
    double acc = 0.0;
    for (int j = w; j < N; j += 4) {
        const double dot = wave_dot(fi, f + (long)j * D, D, lane);
        if (j != i) acc += dot / (norm[i] * norm[j]);
    }
    if (lane == 0) red[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[i] = ((red[0] + red[1]) + red[2]) + red[3];
    if (text && w == 0) {
        const double dot = wave_dot(fi, text, D, lane);
        if (lane == 0) tpart[i] = dot / (norm[i] * norm[N]);
    }
}

// out[0] = sum(part) / (N (N - 1)), out[1] = sum(tpart) / N, each summed in index order by one thread per figure
__global__ __launch_bounds__(64) void k_scores_final(const double* __restrict__ part, const double* __restrict__ tpart, int N, int has_text,
                                                     double* __restrict__ out) {
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += part[i];
        out[0] = N > 1 ? s / ((double)N * (double)(N - 1)) : 0.0;
    } else if (threadIdx.x == 1) {
        double s = 0.0;
        if (has_text) for (int i = 0; i < N; ++i) s += tpart[i];
        out[1] = has_text ? s / (double)N : 0.0;
    }
}

// PickScore (eval_utils.py:163-176): out[1 + i] = exp(logit_scale) <text / |text|, f_i / |f_i|>, one wave per image
__global__ __launch_bounds__(64) void k_pick_row(const float* __restrict__ f, const float* __restrict__ text, int D, double scale, double* __restrict__ out) {
    const int i = blockIdx.x;
    const float* fi = f + (long)i * D;
    const double ff = wave_dot(fi, fi, D, threadIdx.x), tt = wave_dot(text, text, D, threadIdx.x), ft = wave_dot(fi, text, D, threadIdx.x);
    if (threadIdx.x == 0) out[1 + i] = scale * (ft / (sqrt(ff) * sqrt(tt)));
}

// out[0] = the mean of out[1 .. N], summed in index order by one thread
__global__ __launch_bounds__(64) void k_pick_mean(int N, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < N; ++i) s += out[1 + i];
    out[0] = s / (double)N;
}

int preprocess_launch(const void* frames, void* crop, void* patches, int N, int H, int W, int side, int patch, int ldp, int rule, hipStream_t st) {
    TCL_CHECK_ARG(frames && (crop || patches) && N > 0 && N <= 65535 && H > 0 && W > 0 && side > 0 && patch > 0 && (long)H * W < (1L << 28));
    TCL_CHECK_ARG(!patches || side % patch == 0);
    int g[4];
    if (tcl_clip_resize_geometry_rule(H, W, side, rule, g) != TCL_OK) return TCL_EINVAL;
    const Axis ay = make_axis(H, g[0], g[2]), ax = make_axis(W, g[1], g[3]);
    const int max_rows = (int)((PT - 1) * ay.scale + 2.0 * ay.support) + 3;
    const size_t lds = (size_t)(PT * (ax.ksize + ay.ksize) + 4 * PT) * sizeof(int) + (size_t)max_rows * PT * 3;
    TCL_CHECK_ARG(lds <= 64 * 1024);                    // down-scale factors up to about 17
    const int tiles = cdiv(side, PT);
    hipLaunchKernelGGL(k_clip_preprocess, dim3(tiles, tiles, N), dim3(256), lds, st, (const uint8_t*)frames, (uint8_t*)crop, (_Float16*)patches, H, W,
                       side, patch, ldp, ax, ay, max_rows);
    TCL_LAUNCH_RET();
}

}  // namespace

extern "C" {

int tcl_clip_resize_geometry(int H, int W, int side, int* geom) { return tcl_clip_resize_geometry_rule(H, W, side, 0, geom); }

int tcl_clip_resize_geometry_rule(int H, int W, int side, int rule, int* geom) {
    TCL_CHECK_ARG(geom && H > 0 && W > 0 && side > 0 && (rule == 0 || rule == 1));
    const int shrt = W <= H ? W : H, lng = W <= H ? H : W;
    const int nl = (int)((double)((long)side * lng) / (double)shrt);
    const int ow = W <= H ? side : nl, oh = W <= H ? nl : side;
    geom[0] = oh; geom[1] = ow;
    if (rule == 0) {
        geom[2] = (int)nearbyint((oh - side) / 2.0);    // round half to even, as Python's round()
        geom[3] = (int)nearbyint((ow - side) / 2.0);
    } else {
        geom[2] = (oh - side) / 2;                      // transformers center_crop: (size - side) // 2; oh, ow >= side
        geom[3] = (ow - side) / 2;
    }
    return TCL_OK;
}

int tcl_clip_preprocess_u8(const void* frames, void* crop, void* patches, int N, int H, int W, int side, int patch, hipStream_t st) {
    return preprocess_launch(frames, crop, patches, N, H, W, side, patch, 3 * patch * patch, 0, st);
}

int tcl_clip_preprocess_ld_u8(const void* frames, void* crop, void* patches, int N, int H, int W, int side, int patch, int ldp, int rule, hipStream_t st) {
    TCL_CHECK_ARG(patch > 0 && patch <= 1024 && ldp >= 3 * patch * patch && (ldp % 64 == 0 || ldp == 3 * patch * patch) && (rule == 0 || rule == 1));
    return preprocess_launch(frames, crop, patches, N, H, W, side, patch, ldp, rule, st);
}

int tcl_clip_attention_f16(const void* qkv, void* out, int B, int T, int H, int d, float scale, int causal, hipStream_t st) {
    TCL_CHECK_ARG(qkv && out && B > 0 && H > 0 && T > 0 && T <= 288 && d >= 16 && d <= 128 && d % 16 == 0 && (long)B * H < (1L << 31));
    const _Float16* x = (const _Float16*)qkv;
    _Float16* o = (_Float16*)out;
    if (T <= 64) return launch_attn<2>(x, o, B, T, H, d, scale, causal, st);
    if (T <= 96) return launch_attn<3>(x, o, B, T, H, d, scale, causal, st);
    if (T <= 160) return launch_attn<5>(x, o, B, T, H, d, scale, causal, st);
    return launch_attn<9>(x, o, B, T, H, d, scale, causal, st);
}

int tcl_clip_embed_f16(const void* patch, const void* cls, const int* ids, const void* table, const void* pos, const void* gamma, const void* beta,
                       void* out, int B, int T, int W, int vocab, float eps, hipStream_t st) {
    TCL_CHECK_ARG(pos && out && B > 0 && T > 0 && W > 0 && W <= 256 * EMB_K && (long)B * T < (1L << 31) && (!gamma == !beta));
    TCL_CHECK_ARG(ids ? (table && vocab > 0) : (cls && (patch || T == 1)));
    hipLaunchKernelGGL(k_clip_embed, dim3(B * T), dim3(256), 0, st, (const _Float16*)patch, (const _Float16*)cls, ids, (const _Float16*)table,
                       (const _Float16*)pos, (const _Float16*)gamma, (const _Float16*)beta, (_Float16*)out, T, W, vocab, eps);
    TCL_LAUNCH_RET();
}

int tcl_clip_quick_gelu_f16(const void* x, void* y, long n, hipStream_t st) {
    TCL_CHECK_ARG(x && y && n > 0 && n % 8 == 0);
    hipLaunchKernelGGL(k_quick_gelu, dim3(stream_grid(n / 8)), dim3(256), 0, st, (const _Float16*)x, (_Float16*)y, n / 8);
    TCL_LAUNCH_RET();
}

size_t tcl_clip_scores_workspace_bytes(int N) { return N > 0 ? (size_t)(3 * (size_t)N + 1) * sizeof(double) : 0; }

int tcl_clip_scores(const float* feats, const float* text, int N, int D, double* out2, void* ws, hipStream_t st) {
    TCL_CHECK_ARG(feats && out2 && ws && N > 0 && N <= 65535 && D > 0);
    double* norm = (double*)ws;
    double* part = norm + N + 1;
    double* tpart = part + N;
    hipLaunchKernelGGL(k_scores_norm, dim3(N + (text ? 1 : 0)), dim3(64), 0, st, feats, text, N, D, norm);
    hipLaunchKernelGGL(k_scores_row, dim3(N), dim3(256), 0, st, feats, text, N, D, (const double*)norm, part, tpart);
    hipLaunchKernelGGL(k_scores_final, dim3(1), dim3(64), 0, st, (const double*)part, (const double*)tpart, N, text ? 1 : 0, out2);
    TCL_LAUNCH_RET();
}

int tcl_pick_scores(const float* feats, const float* text, int N, int D, float logit_scale, double* out, hipStream_t st) {
    TCL_CHECK_ARG(feats && text && out && N > 0 && N <= 65535 && D > 0);
    hipLaunchKernelGGL(k_pick_row, dim3(N), dim3(64), 0, st, feats, text, D, exp((double)logit_scale), out);
    hipLaunchKernelGGL(k_pick_mean, dim3(1), dim3(64), 0, st, N, out);
    TCL_LAUNCH_RET();
}

}  // extern "C"
