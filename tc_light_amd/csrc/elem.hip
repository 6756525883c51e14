// HBM-bound f16 kernels of path 1 (gfx950): GroupNorm(+SiLU), LayerNorm, GEGLU, row softmax, channel concat,
// small-Cin im2col, GEMV (time embedding), latent pack/unpack with classifier-free guidance, AdaIN + noise fusion,
// SDE-DPM-Solver++ update, DDIM inversion pack / step (f32 master latents), image<->latent layout conversion.  All loads/stores are 16 B per lane (8 halves)
// unless a kernel says otherwise.
// Reference call sites: UNet/VAE norms via diffusers (generate.py:342-347); pred_noise generate.py:288-352;
// temporal_denoise :241-284; adaptive_instance_normalization utils/general_utils.py:137-156;
// scheduler.step generate.py:235; encode/decode_latents utils/VidToMe/generate_utils.py:140-172; Inverter.pred_next_x invert.py:215-244.
#include "common.h"
#include "../../include/tclight_hip.h"
#include <unordered_map>

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------ GroupNorm
// pass 1: per-(batch, group) sum / sumsq of x = [x1 | x2] (channel concat, x2 may be null), DETERMINISTIC: no float atomics anywhere.
// Each block reduces its row range to one partial per group -- every thread owns one 8-channel chunk (at most two groups, split at a
// per-thread constant) and walks rows; the per-thread partials go to LDS and thread g adds up, in a fixed order, exactly the
// entries that belong to group g -- and writes part[b][block][g]; k_gn_reduce then sums the blocks in order.
__global__ __launch_bounds__(256) void k_gn_stats(const _Float16* __restrict__ x1, int C1, const _Float16* __restrict__ x2, int C2,
                                                  int HW, int G, int rows_per_block, float* __restrict__ part) {
    __shared__ float ps[256][4];
    const int b = blockIdx.y, C = C1 + C2, cpg = C / G, nchunk = C / 8;
    const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, HW);
    const int cw = nchunk < 256 ? nchunk : 256, rp = 256 / cw;
    const int tc = threadIdx.x % cw, tr = threadIdx.x / cw;
    float gsum = 0.f, gsq = 0.f;                                  // group threadIdx.x (< G) of this block
    for (int c0 = 0; c0 < nchunk; c0 += cw) {
        const int chunk = c0 + tc;
        float sa = 0, qa = 0, sl = 0, ql = 0;                     // all 8 channels / the part in the chunk's first group
        if (tr < rp && chunk < nchunk) {
            const int ch = chunk * 8, gf = ch / cpg;
            float wlo[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) wlo[j] = ((ch + j) / cpg == gf) ? 1.f : 0.f;
            const bool first = ch < C1;
            const _Float16* base = first ? x1 + (long)b * HW * C1 + ch : x2 + (long)b * HW * C2 + (ch - C1);
            const int ld = first ? C1 : C2;
            // 4 loads in flight per thread (the first form waited for every 16-byte load before issuing the next: latency-bound at ~3.8 TB/s): full
            // groups of 4 rows without a guard, then the tail row by row -- the accumulation order (row by row, channel by channel) is unchanged
            auto acc = [&](const h8& v) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float f = (float)v[j], f2 = f * f;
                    sa += f; qa += f2; sl += f * wlo[j]; ql += f2 * wlo[j];
                }
            };
            int row = r0 + tr;
            for (; row + 3 * rp < r1; row += 4 * rp) {
                h8 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *(const h8*)(base + (long)(row + u * rp) * ld);
#pragma unroll
                for (int u = 0; u < 4; ++u) asm volatile("" :: "v"(v[u]));      // all four issued before the first is consumed (the scheduler otherwise trickles them in two at a time behind the serial sums)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc(v[u]);
            }
            for (; row < r1; row += rp) acc(*(const h8*)(base + (long)row * ld));
        }
        __syncthreads();
        ps[threadIdx.x][0] = sl; ps[threadIdx.x][1] = ql; ps[threadIdx.x][2] = sa - sl; ps[threadIdx.x][3] = qa - ql;
        __syncthreads();
        if (threadIdx.x < G) {
            // chunks that touch group g: floor(g*cpg/8) .. floor(((g+1)*cpg-1)/8), restricted to this c0 window
            const int g = threadIdx.x, clo = max(g * cpg / 8, c0), chi = min(min(((g + 1) * cpg - 1) / 8, nchunk - 1), c0 + cw - 1);
            for (int cc = clo; cc <= chi; ++cc) {
                const int gf = cc * 8 / cpg;                          // first group of that chunk: its head goes to gf, its tail to gf + 1
                for (int rr = 0; rr < rp; ++rr) {
                    const float* e = ps[rr * cw + (cc - c0)];
                    if (gf == g) { gsum += e[0]; gsq += e[1]; } else { gsum += e[2]; gsq += e[3]; }
                }
            }
        }
    }
    if (threadIdx.x < G) {
        float* o = part + (((long)b * gridDim.x + blockIdx.x) * 64 + threadIdx.x) * 2;
        o[0] = gsum; o[1] = gsq;
    }
}
// pass 1b: sums[b][g] = sum over the blocks in a fixed order: 8 interleaved partial sums per output, combined 0..7
__global__ __launch_bounds__(1024) void k_gn_reduce(const float* __restrict__ part, int nblk, int G, float* __restrict__ sums) {
    __shared__ float red[8][128];
    const int b = blockIdx.x, o = threadIdx.x & 127, p = threadIdx.x >> 7;        // o = g*2 + k
    float s = 0.f;
    if (o < 2 * G) {
        const float* src = part + (long)b * nblk * 128 + o;
#pragma unroll 4
        for (int i = p; i < nblk; i += 8) s += src[(long)i * 128];
    }
    red[p][o] = s;
    __syncthreads();
    if (p == 0 && o < 2 * G) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += red[q][o];
        sums[(long)b * G * 2 + o] = t;
    }
}
// pass 2: y = act((x - mean) * rstd * gamma + beta) with the per-(batch, group) statistics folded in per 8-channel chunk (a chunk
// touches at most two groups); also materialises the channel concat.
template <bool SILU, bool RAW>
__global__ __launch_bounds__(256) void k_gn_apply(const _Float16* __restrict__ x1, int C1, const _Float16* __restrict__ x2, int C2,
                                                  const float* __restrict__ sums, const _Float16* __restrict__ gamma,
                                                  const _Float16* __restrict__ beta, float inv_n, float eps, int G, _Float16* __restrict__ y, int HW,
                                                  _Float16* __restrict__ yraw) {
    // Round 5: a thread OWNS one 8-channel chunk and walks rows (threads of a block: [rows rp][chunks cw], consecutive lanes = consecutive chunks of a
    // row), so the per-channel scale / shift -- two statistics loads, two rsqrt, gamma / beta -- is built once per thread instead of once per 16 bytes
    // (the first form spent ~140 vector instructions per chunk, most of them on constants: it was as VALU-bound as HBM-bound).  Same arithmetic per element.
    // Round 5, second pass: the row walk keeps GN_U loads in flight per thread (the ISA of the first form was load -> s_waitcnt vmcnt(0) -> 8 branches on
    // the run-time `silu` -> store: ONE 16-byte load in flight per thread = 32 KB per CU, ~4 TB/s by Little's law at 2 us of loaded HBM latency);
    // full groups of GN_U rows run without any guard (a guard at the store made hipcc sink each load into its guarded region again), the tail row by row.
    constexpr int GN_U = 4;
    const int b = blockIdx.y, C = C1 + C2, nchunk = C / 8, cpg = C / G;
    const int cw = nchunk < 256 ? nchunk : 256, rp = 256 / cw;
    const int tc = threadIdx.x % cw, tr = threadIdx.x / cw;
    if (tr >= rp) return;
    for (int c0 = 0; c0 < nchunk; c0 += cw) {
        const int chunk = c0 + tc;
        if (chunk >= nchunk) continue;
        const int ch = chunk * 8;
        const h8 ga = *(const h8*)(gamma + ch), be = *(const h8*)(beta + ch);
        const int g0 = ch / cpg, g1 = (ch + 7) / cpg, split = (g0 + 1) * cpg - ch;      // channels j >= split belong to g1
        const float2 s0 = *(const float2*)(sums + ((long)b * G + g0) * 2), s1 = *(const float2*)(sums + ((long)b * G + g1) * 2);
        const float m0 = s0.x * inv_n, m1 = s1.x * inv_n;
        const float r0 = rsqrtf(fmaxf(s0.y * inv_n - m0 * m0, 0.f) + eps), r1 = rsqrtf(fmaxf(s1.y * inv_n - m1 * m1, 0.f) + eps);
        float sc[8], sh[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float mean = j < split ? m0 : m1, rstd = j < split ? r0 : r1;
            sc[j] = rstd * (float)ga[j]; sh[j] = (float)be[j] - mean * sc[j];
        }
        const bool first = ch < C1;
        const _Float16* base = first ? x1 + (long)b * HW * C1 + ch : x2 + (long)b * HW * C2 + (ch - C1);
        const int ld = first ? C1 : C2;
        _Float16* yb = y + (long)b * HW * C + ch;
        _Float16* rb = RAW ? yraw + (long)b * HW * C + ch : nullptr;
        const int step = gridDim.x * rp;
        auto apply = [&](const h8& v, int r) {
            h8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float a = (float)v[j] * sc[j] + sh[j];
                if (SILU) a = a / (1.f + __expf(-a));
                o[j] = (_Float16)a;
            }
            *(h8*)(yb + (long)r * C) = o;
            if (RAW) *(h8*)(rb + (long)r * C) = v;      // the un-normalised concat, for the ResNet block's 1x1 shortcut (round 5: was a pass of its own)
        };
        int row = blockIdx.x * rp + tr;
        for (; row + (GN_U - 1) * step < HW; row += GN_U * step) {      // full groups: no guard anywhere, the GN_U loads are issued back to back
            h8 v[GN_U];
#pragma unroll
            for (int u = 0; u < GN_U; ++u) v[u] = *(const h8*)(base + (long)(row + u * step) * ld);
            // (the RAW form issues rows 3 and 4 behind the stores of rows 1 and 2; pinning all four ahead of the first store measured no gain -- 705 / 1 029 / 522 us
            // against 709 / 1 035 / 533 pinned on one box, tools/micro/gn_raw_check.py -- the pass is at the HBM rate either way)
#pragma unroll
            for (int u = 0; u < GN_U; ++u) apply(v[u], row + u * step);
        }
        for (; row < HW; row += step) apply(*(const h8*)(base + (long)row * ld), row);
    }
}

// ------------------------------------------------------------------------------------------ LayerNorm (one wave per row)
// METRIC: also write the row's cosine-normalised form y / |y| for the VidToMe matching of this block (merge.py:84: metric / metric.norm()),
// with exactly the arithmetic and summation order of merge.hip::k_tome_normalize on the f16 y -- same lane <-> chunk layout -- so the
// matching sees the same bits as when it normalised the tokens itself (one launch and one read of the tokens less per chunk and block).
// Round 5, second pass: a wave takes LN_R consecutive rows and issues all their loads before the first reduction (the first form had one row per
// wave and, for C = 320, ONE 16-byte load in flight on 40 of the 64 lanes: ~2.9 TB/s); NK = ceil(C / 512) chunk slots per lane is a template
// parameter, so there is no branch around a load (chunk and row are clamped for the load, masked in the sums and at the store).  Per row the
// arithmetic, the lane <-> chunk layout and the summation order are those of the first form: same bits.
#define LN_R 4
template <bool METRIC, int NK>
__global__ __launch_bounds__(256) void k_layernorm(const _Float16* __restrict__ x, const _Float16* __restrict__ gamma,
                                                   const _Float16* __restrict__ beta, _Float16* __restrict__ y, _Float16* __restrict__ metric,
                                                   long rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const long row0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * LN_R;
    if (row0 >= rows) return;
    const int nchunk = C / 8;
    bool ok[NK]; int off[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) { const int ch = lane + 64 * k; ok[k] = ch < nchunk; off[k] = min(ch, nchunk - 1) * 8; }
    h8 v[LN_R][NK];
#pragma unroll
    for (int r = 0; r < LN_R; ++r) {
        const _Float16* xr = x + min(row0 + r, rows - 1) * C;
#pragma unroll
        for (int k = 0; k < NK; ++k) v[r][k] = *(const h8*)(xr + off[k]);
    }
    h8 g[NK], bt[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) { g[k] = *(const h8*)(gamma + off[k]); bt[k] = *(const h8*)(beta + off[k]); }
#pragma unroll
    for (int r = 0; r < LN_R; ++r) {
        const long row = row0 + r;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (ok[k])
#pragma unroll
                for (int j = 0; j < 8; ++j) s += (float)v[r][k][j];
        const float mean = wave_sum(s) / C;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (ok[k])
#pragma unroll
                for (int j = 0; j < 8; ++j) { float d = (float)v[r][k][j] - mean; q += d * d; }
        const float rstd = rsqrtf(wave_sum(q) / C + eps);
        float q2 = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            h8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (_Float16)(((float)v[r][k][j] - mean) * rstd * (float)g[k][j] + (float)bt[k][j]);
            if (ok[k] && row < rows) *(h8*)(y + row * C + off[k]) = o;
            if (METRIC) {
                v[r][k] = o;
                if (ok[k])
#pragma unroll
                    for (int j = 0; j < 8; ++j) q2 += (float)o[j] * (float)o[j];
            }
        }
        if (METRIC) {
            const float nrm = (float)(_Float16)sqrtf(wave_sum(q2));
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                h8 o;
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (_Float16)((float)v[r][k][j] / nrm);
                if (ok[k] && row < rows) *(h8*)(metric + row * C + off[k]) = o;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ GEGLU: out = a * gelu(gate)
__global__ void k_geglu(const _Float16* __restrict__ in, _Float16* __restrict__ out, long rows, int D) {
    const int nchunk = D / 8;
    const long total = rows * nchunk;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long r = i / nchunk; int ch = (int)(i % nchunk) * 8;
        h8 a = *(const h8*)(in + r * 2 * D + ch), g = *(const h8*)(in + r * 2 * D + D + ch), o;
#pragma unroll
        for (int j = 0; j < 8; ++j) { float gf = (float)g[j]; o[j] = (_Float16)((float)a[j] * (0.5f * gf * (1.f + erff(gf * 0.70710678f)))); }
        *(h8*)(out + r * D + ch) = o;
    }
}

// ------------------------------------------------------------------------------------------ row softmax (in place, scaled)
__global__ __launch_bounds__(256) void k_softmax_rows(_Float16* __restrict__ x, int T, int ld, float scale) {
    extern __shared__ float rowbuf[];
    __shared__ float red[16];
    _Float16* p = x + (long)blockIdx.x * ld;
    float mx = -1e30f;
    for (int i = threadIdx.x; i < T; i += 256) { float v = (float)p[i] * scale; rowbuf[i] = v; mx = fmaxf(mx, v); }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = 0.f;
    for (int i = threadIdx.x; i < T; i += 256) { float e = __expf(rowbuf[i] - mx); rowbuf[i] = e; s += e; }
    float tot = block_sum(s, red + 4);
    __shared__ float inv;
    if (threadIdx.x == 0) inv = 1.f / tot;
    __syncthreads();
    for (int i = threadIdx.x; i < T; i += 256) p[i] = (_Float16)(rowbuf[i] * inv);
}

// The same with the row in REGISTERS (round 5): 16-byte loads / stores, up to 8 chunks of 8 per thread (T <= 16 384, T and ld multiples of 8) -- the LDS form
// above moves 2 bytes per lane and instruction and ran the VAE mid-block's 14 400 x 14 400 score matrix at 0.95 TB/s (870 us per frame).
__global__ __launch_bounds__(256) void k_softmax_rows_reg(_Float16* __restrict__ x, int T, int ld, float scale) {
    __shared__ float red[32];
    _Float16* p = x + (long)blockIdx.x * ld;
    const int nchunk = T / 8;
    float v[8][8];
    float mx = -1e30f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = threadIdx.x + 256 * k;
        if (c < nchunk) {
            const h8 h = *(const h8*)(p + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) { v[k][j] = (float)h[j] * scale; mx = fmaxf(mx, v[k][j]); }
        }
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (threadIdx.x + 256 * k < nchunk)
#pragma unroll
            for (int j = 0; j < 8; ++j) { v[k][j] = __expf(v[k][j] - mx); s += v[k][j]; }
    const float tot = block_sum(s, red + 8);
    if (threadIdx.x == 0) red[4] = 1.f / tot;
    __syncthreads();
    const float inv = red[4];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = threadIdx.x + 256 * k;
        if (c < nchunk) {
            h8 h;
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = (_Float16)(v[k][j] * inv);
            *(h8*)(p + c * 8) = h;
        }
    }
}

// ------------------------------------------------------------------------------------------ small helpers
__global__ void k_concat(const _Float16* __restrict__ x1, int C1, const _Float16* __restrict__ x2, int C2, _Float16* __restrict__ y, long rows) {
    const int nchunk = (C1 + C2) / 8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < rows * nchunk; i += (long)gridDim.x * blockDim.x) {
        long r = i / nchunk; int ch = (int)(i % nchunk) * 8;
        *(h8*)(y + r * (C1 + C2) + ch) = ch < C1 ? *(const h8*)(x1 + r * C1 + ch) : *(const h8*)(x2 + r * C2 + ch - C1);
    }
}
// [B,H,W,Cin] -> [B*Ho*Wo, Kpad] im2col for 3x3 convs with tiny Cin (conv_in 8->320, VAE 3->128 / 4->512)
__global__ void k_im2col_small(const _Float16* __restrict__ x, _Float16* __restrict__ out, int B, int H, int W, int Cin, int Kpad) {
    const long total = (long)B * H * W * Kpad;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int k = (int)(i % Kpad); long m = i / Kpad;
        _Float16 v = (_Float16)0.f;
        if (k < 9 * Cin) {
            int tap = k / Cin, c = k - tap * Cin, ky = tap / 3, kx = tap - ky * 3;
            int xx = (int)(m % W), yy = (int)((m / W) % H); long b = m / ((long)W * H);
            int iy = yy + ky - 1, ix = xx + kx - 1;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[((b * H + iy) * W + ix) * Cin + c];
        }
        out[i] = v;
    }
}
// y[n] = act(W[n,:] . x + b[n]) -- one wave per output (time-embedding MLP, per-ResBlock time projection)
__global__ __launch_bounds__(256) void k_gemv(const _Float16* __restrict__ W, const _Float16* __restrict__ x, const _Float16* __restrict__ bias,
                                              const _Float16* __restrict__ add, _Float16* __restrict__ y, int N, int K, int silu_in, int silu_out) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    float s = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        h8 w = *(const h8*)(W + (long)n * K + k), v = *(const h8*)(x + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) { float xv = (float)v[j]; if (silu_in) xv = (float)(_Float16)(xv / (1.f + __expf(-xv))); s += (float)w[j] * xv; }
    }
    s = wave_sum(s);
    if (lane == 0) {
        s += bias ? (float)bias[n] : 0.f;
        if (silu_out) s = s / (1.f + __expf(-s));
        if (add) s = (float)(_Float16)s + (float)add[n];
        y[n] = (_Float16)s;
    }
}
// sinusoidal timestep embedding, flip_sin_to_cos=True, freq_shift=0 (diffusers Timesteps): [cos | sin], dim 320
__global__ void k_timestep_embed(float t, int dim, _Float16* __restrict__ out) {
    const int i = threadIdx.x, half = dim / 2;
    if (i >= half) return;
    float freq = __expf(-logf(10000.f) * (float)i / (float)half);
    out[i] = (_Float16)cosf(t * freq); out[half + i] = (_Float16)sinf(t * freq);
}

// ------------------------------------------------------------------------------------------ latent pack / unpack
// mode 0 (xy, generate.py:220-224): image j = frame idx[j];   out[b*F + j][y][x][c] (c<4: x, c>=4: concat_conds), b = 0,1
// mode 1 (yt, generate.py:267-273 'n c h w -> w c n h'): image j = latent column idx[j], rows = frames sl..sl+nwin, cols = h
__global__ void k_pack_latents(const _Float16* __restrict__ x, const _Float16* __restrict__ cond, const int* __restrict__ idx, int F,
                               int mode, int sl, int nwin, int h, int w, _Float16* __restrict__ out) {
    const int Hh = mode ? nwin : h, Ww = mode ? h : w;
    const long per = (long)Hh * Ww, total = (long)F * per;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int j = (int)(i / per); long r = i % per; int yy = (int)(r / Ww), xx = (int)(r % Ww);
        int n = mode ? sl + yy : idx[j], hy = mode ? xx : yy, wx = mode ? idx[j] : xx;
        h8 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            long src = (((long)n * 4 + c) * h + hy) * w + wx;
            v[c] = x[src]; v[4 + c] = cond[src];
        }
        *(h8*)(out + ((long)j * per + r) * 8) = v;
        *(h8*)(out + ((long)(F + j) * per + r) * 8) = v;
    }
}
// 12-channel records of the background-conditioned IC-Light model (utils/model_utils.py:97-179, init_iclight_bg): x | cond_fg | cond_bg, 24 B per
// pixel, written as one 16 B and one 8 B store, the 16 B one on whichever side of the record is 16 B aligned (`out` is 8 B aligned: host check).
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_rec12(_Float16* p, h4 a, h4 b, h4 c) {
    if (((uintptr_t)p & 15) == 0) {
        *(h8*)p = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); *(h4*)(p + 8) = c;
    } else {
        *(h4*)p = a; *(h8*)(p + 4) = __builtin_shufflevector(b, c, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}
// xy: image j = frame idx[j].  One lane per pixel, consecutive lanes on consecutive wx: every one of the 12 NCHW plane reads is a contiguous
// 128 B per wave; a lane's record goes out twice (uncond, cond half).  bg_one: the single background latent serves every frame.
__global__ __launch_bounds__(256) void k_pack_latents12_xy(const _Float16* __restrict__ x, const _Float16* __restrict__ fg,
                                                           const _Float16* __restrict__ bg, int bg_one, const int* __restrict__ idx, int F,
                                                           int h, int w, _Float16* __restrict__ out) {
    const long per = (long)h * w, total = (long)F * per;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i / per); const long r = i - (long)j * per;
        const long n = idx[j], nb = bg_one ? 0 : n;
        h4 a, b, c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a[k] = x[(n * 4 + k) * per + r]; b[k] = fg[(n * 4 + k) * per + r]; c[k] = bg[(nb * 4 + k) * per + r];
        }
        store_rec12(out + ((long)j * per + r) * 12, a, b, c);
        store_rec12(out + ((long)(F + j) * per + r) * 12, a, b, c);
    }
}
// yt ('n c h w -> w c n h'): image j = latent column idx[j], rows = frames sl..sl+nwin, cols = hy.  The output runs along hy, the NCHW source
// along wx = idx[j], so a tile of PK12_T columns x PK12_T rows of one frame is transposed through LDS: read with consecutive lanes on consecutive
// j (a chunk's columns are consecutive: contiguous 64 B runs), written with consecutive lanes on consecutive hy (contiguous 24 B records).
// LDS row stride 12*PK12_T + 4 halves = 194 dwords: the 32 lanes of a read-phase row land in 32 different banks, records stay 8 B aligned.
#define PK12_T 32
#define PK12_LD (12 * PK12_T + 4)
__global__ __launch_bounds__(256) void k_pack_latents12_yt(const _Float16* __restrict__ x, const _Float16* __restrict__ fg,
                                                           const _Float16* __restrict__ bg, int bg_one, const int* __restrict__ idx, int F,
                                                           int sl, int nwin, int h, int w, _Float16* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) _Float16 tile[PK12_T * PK12_LD];
    const int tj = (F + PK12_T - 1) / PK12_T, th = (h + PK12_T - 1) / PK12_T;
    const long tiles = (long)nwin * tj * th, plane = (long)h * w, per = (long)nwin * h;
    const int lo = threadIdx.x & (PK12_T - 1), hi = threadIdx.x >> 5;          // 256 threads: 32 x 8
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {                     // block-uniform trip count: the barriers below are safe
        const int yy = (int)(t / ((long)tj * th)), rem = (int)(t - (long)yy * tj * th);
        const int j0 = (rem / th) * PK12_T, h0 = (rem % th) * PK12_T;
        const long n = sl + yy, nb = bg_one ? 0 : n;
        {   // read phase: lane -> column j0 + lo, rows h0 + hi, hi + 8, ...
            const int j = j0 + lo;
            const int wx = j < F ? idx[j] : 0;
#pragma unroll
            for (int p = 0; p < PK12_T / 8; ++p) {
                const int hl = p * 8 + hi, hy = h0 + hl;
                const bool ok = j < F && hy < h;
                _Float16* d = tile + lo * PK12_LD + hl * 12;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long off = (long)hy * w + wx;
                    d[k] = ok ? x[(n * 4 + k) * plane + off] : (_Float16)0.f;
                    d[4 + k] = ok ? fg[(n * 4 + k) * plane + off] : (_Float16)0.f;
                    d[8 + k] = ok ? bg[(nb * 4 + k) * plane + off] : (_Float16)0.f;
                }
            }
        }
        __syncthreads();
        {   // write phase: lane -> row h0 + lo, columns j0 + hi, hi + 8, ...
            const int hy = h0 + lo;
#pragma unroll
            for (int p = 0; p < PK12_T / 8; ++p) {
                const int jl = p * 8 + hi, j = j0 + jl;
                if (j < F && hy < h) {
                    const _Float16* s = tile + jl * PK12_LD + lo * 12;
                    const h4 a = *(const h4*)s, b = *(const h4*)(s + 4), c = *(const h4*)(s + 8);
                    const long r = (long)yy * h + hy;
                    store_rec12(out + ((long)j * per + r) * 12, a, b, c);
                    store_rec12(out + ((long)(F + j) * per + r) * 12, a, b, c);
                }
            }
        }
        __syncthreads();
    }
}
// eps [2F, Hh, Ww, 4] -> noise[n][c][hy][wx] = (u + g*(c - u)) * scale(frame)   (generate.py:349-350, :273-278)
__global__ void k_unpack_cfg(const _Float16* __restrict__ eps, const int* __restrict__ idx, int F, int mode, int sl, int nwin, int h, int w,
                             float guidance, int scale_upto, float scale, int nkeep, _Float16* __restrict__ noise) {
    const int Hh = mode ? nwin : h, Ww = mode ? h : w;
    const long per = (long)Hh * Ww, total = (long)F * per;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int j = (int)(i / per); long r = i % per; int yy = (int)(r / Ww), xx = (int)(r % Ww);
        if (mode && yy >= nkeep) continue;   // frames the next window overwrites anyway (generate.py:265-278)
        int n = mode ? sl + yy : idx[j], hy = mode ? xx : yy, wx = mode ? idx[j] : xx;
        const _Float16* u = eps + ((long)j * per + r) * 4; const _Float16* c = eps + ((long)(F + j) * per + r) * 4;
        float sc = (mode && n < scale_upto) ? scale : 1.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float uu = (float)u[k], v = uu + guidance * ((float)c[k] - uu);
            noise[(((long)n * 4 + k) * h + hy) * w + wx] = (_Float16)(v * sc);
        }
    }
}

// ------------------------------------------------------------------------------------------ AdaIN + fusion (one block per (n,c) plane)
// nt <- AdaIN(nt, nxy) ; nxy <- sqrt(alpha)*nt + sqrt(1-alpha)*nxy      (generate.py:281-282)
__global__ __launch_bounds__(256) void k_adain_fuse(_Float16* __restrict__ nt, _Float16* __restrict__ nxy, int hw, float alpha) {
    __shared__ float red[16]; __shared__ float st[4];
    _Float16* a = nt + (long)blockIdx.x * hw; _Float16* b = nxy + (long)blockIdx.x * hw;
    float sa = 0, sb = 0;
    for (int i = threadIdx.x; i < hw; i += 256) { sa += (float)a[i]; sb += (float)b[i]; }
    float ta = block_sum(sa, red); if (threadIdx.x == 0) st[0] = ta / hw;
    float tb = block_sum(sb, red); if (threadIdx.x == 0) st[1] = tb / hw;
    __syncthreads();
    const float ma = st[0], mb = st[1];
    float qa = 0, qb = 0;
    for (int i = threadIdx.x; i < hw; i += 256) { float d = (float)a[i] - ma; qa += d * d; d = (float)b[i] - mb; qb += d * d; }
    ta = block_sum(qa, red); if (threadIdx.x == 0) st[2] = sqrtf(ta / (hw - 1) + 1e-5f);
    tb = block_sum(qb, red); if (threadIdx.x == 0) st[3] = sqrtf(tb / (hw - 1) + 1e-5f);
    __syncthreads();
    const float sda = st[2], sdb = st[3], wa = sqrtf(alpha), wb = sqrtf(1.f - alpha);
    for (int i = threadIdx.x; i < hw; i += 256) {
        float v = ((float)a[i] - ma) / sda * sdb + mb, o = (float)b[i];
        _Float16 vh = (_Float16)v;
        a[i] = vh; b[i] = (_Float16)(wa * (float)vh + wb * o);
    }
}

// ------------------------------------------------------------------------------------------ SDE-DPM-Solver++(2M) update (f32 math)
// x0 = (x - sigma_t*eps)/alpha_t is stored in m0 (f32); x_next = ca*x + cb*(D) + cc*z with D = m0 (order 1)
// or D = m0 + r1*(m0 - m1) folded on the host into (cb0, cb1).
__global__ void k_dpm_step(_Float16* __restrict__ x, const _Float16* __restrict__ eps, float* __restrict__ m0, const float* __restrict__ m1,
                           const _Float16* __restrict__ z, long n, float sigma_t, float alpha_t, float ca, float cb0, float cb1, float cc) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float xv = (float)x[i], x0 = (xv - sigma_t * (float)eps[i]) / alpha_t;
        float prev = m1 ? m1[i] : 0.f;
        m0[i] = x0;
        float r = ca * xv + cb0 * x0 + cb1 * prev + (z ? cc * (float)z[i] : 0.f);
        x[i] = (_Float16)r;
    }
}

// ------------------------------------------------------------------------------------------ DDIM inversion (invert.py:151-244)
// One lane per pixel of one slot: slot j serves frame idx[j]; a slot whose frame id is outside [0, N) is skipped (nothing read or written).
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

// master x [N,4,hw] f32, cond [N,4,hw] f16 -> out [F,hw,8] f16: channels 0-3 = f16(x), 4-7 = cond
__global__ void k_invert_pack(const float* __restrict__ x, const _Float16* __restrict__ cond, const int* __restrict__ idx, int N, int F, long hw,
                              _Float16* __restrict__ out) {
    const long total = (long)F * hw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long j = i / hw, p = i - j * hw;
        const int n = idx[j];
        if (n < 0 || n >= N) continue;
        h8 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long src = ((long)n * 4 + c) * hw + p;
            v[c] = (_Float16)x[src]; v[4 + c] = cond[src];
        }
        *(h8*)(out + i * 8) = v;
    }
}

// pred_next_x (invert.py:237-242) on the f32 master planes of the first F_valid slots, in place:
//   x0 = (x - s_a*eps) / m_a ; x = m_b*x0 + s_b*eps        every product, difference, quotient and sum rounded to f32 on its own
// and f16(x) into channels 0-3 of the slot's UNet input record (channels 4-7 stay as k_invert_pack wrote them).
__global__ void k_ddim_step(float* __restrict__ x, const _Float16* __restrict__ eps, const int* __restrict__ idx, int N, int F_valid, long hw,
                            float s_a, float m_a, float m_b, float s_b, _Float16* __restrict__ xin) {
#pragma clang fp contract(off)
    const long total = (long)F_valid * hw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long j = i / hw, p = i - j * hw;
        const int n = idx[j];
        if (n < 0 || n >= N) continue;
        const h4 e = *(const h4*)(eps + i * 4);
        h4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float* px = x + ((long)n * 4 + c) * hw + p;
            const float ev = (float)e[c];
            const float se = s_a * ev;
            const float x0 = (*px - se) / m_a;
            const float a = m_b * x0, b = s_b * ev;
            const float xn = a + b;
            *px = xn;
            o[c] = (_Float16)xn;
        }
        *(h4*)(xin + i * 8) = o;
    }
}

// ------------------------------------------------------------------------------------------ image <-> NHWC f16
// img [B,3,H,W] f32 in [0,1] -> out [B,H,W,8] f16 = 2*img-1 (channels 3..7 zero: K padding for the im2col conv)
__global__ void k_img_to_nhwc(const float* __restrict__ img, _Float16* __restrict__ out, int B, int HW) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)B * HW; i += (long)gridDim.x * blockDim.x) {
        long b = i / HW, p = i % HW; h8 v;
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = c < 3 ? (_Float16)(2.f * img[(b * 3 + c) * HW + p] - 1.f) : (_Float16)0.f;
        *(h8*)(out + i * 8) = v;
    }
}
// y [B,HW,ldc] f16 (first 3 channels) -> img [B,3,H,W] f32 = clamp(y/2+0.5, 0, 1)
__global__ void k_nhwc_to_img(const _Float16* __restrict__ y, int ldc, float* __restrict__ img, int B, int HW) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)B * HW; i += (long)gridDim.x * blockDim.x) {
        long b = i / HW, p = i % HW;
#pragma unroll
        for (int c = 0; c < 3; ++c) img[(b * 3 + c) * HW + p] = fminf(fmaxf((float)(_Float16)((float)y[i * ldc + c] * 0.5f + 0.5f), 0.f), 1.f);
    }
}
// generic NHWC f16 [B,HW,ldc] (first C channels, scaled) <-> NCHW f16 [B,C,HW]
__global__ void k_nhwc_to_nchw(const _Float16* __restrict__ y, int ldc, _Float16* __restrict__ out, int B, int C, int HW, float scale) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)B * HW; i += (long)gridDim.x * blockDim.x) {
        long b = i / HW, p = i % HW;
        for (int c = 0; c < C; ++c) out[(b * C + c) * HW + p] = (_Float16)((float)y[i * ldc + c] * scale);
    }
}
__global__ void k_nchw_to_nhwc(const _Float16* __restrict__ x, _Float16* __restrict__ out, int ldc, int B, int C, int HW, float scale) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)B * HW; i += (long)gridDim.x * blockDim.x) {
        long b = i / HW, p = i % HW;
        for (int c = 0; c < ldc; ++c) out[i * ldc + c] = c < C ? (_Float16)((float)x[(b * C + c) * HW + p] * scale) : (_Float16)0.f;
    }
}
// out[T2, T1] = in[T1, T2]^T (row-major f16), batched
__global__ void k_transpose(const _Float16* __restrict__ in, _Float16* __restrict__ out, int R, int Cc, int ldi, int ldo) {
    __shared__ _Float16 t[32][33];
    const long bo = (long)blockIdx.z;
    int x = blockIdx.x * 32 + threadIdx.x, y0 = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += 8) if (x < Cc && y0 + j < R) t[j][threadIdx.x] = in[bo * R * ldi + (long)(y0 + j) * ldi + x];
    __syncthreads();
    int xo = blockIdx.y * 32 + threadIdx.x;
    for (int j = threadIdx.y; j < 32; j += 8) { int yo = blockIdx.x * 32 + j; if (xo < R && yo < Cc) out[bo * Cc * ldo + (long)yo * ldo + xo] = t[threadIdx.x][j]; }
}

__global__ void k_conv1x1_small(const _Float16* __restrict__ x, int ldi, const _Float16* __restrict__ W, const _Float16* __restrict__ b,
                                _Float16* __restrict__ y, int ldo, long M, int Ci, int Co) {
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long)gridDim.x * blockDim.x) {
        float xi[8];
        for (int i = 0; i < Ci; ++i) xi[i] = (float)x[m * ldi + i];
        for (int o = 0; o < ldo; ++o) {
            float a = 0.f;
            if (o < Co) { a = (float)b[o]; for (int i = 0; i < Ci; ++i) a += (float)W[o * Ci + i] * xi[i]; }
            y[m * ldo + o] = (_Float16)a;
        }
    }
}

template <bool METRIC>
static void launch_layernorm(const void* x, const void* gamma, const void* beta, void* y, void* metric, long rows, int C, float eps, hipStream_t st) {
    const dim3 grid(cdiv(rows, 4 * LN_R)), blk(256);
    const int nk = (C / 8 + 63) / 64;
#define LN_GO(NK_) hipLaunchKernelGGL((k_layernorm<METRIC, NK_>), grid, blk, 0, st, (const _Float16*)x, (const _Float16*)gamma, (const _Float16*)beta, \
                                      (_Float16*)y, (_Float16*)metric, rows, C, eps)
    if (nk <= 1) LN_GO(1); else if (nk == 2) LN_GO(2); else if (nk == 3) LN_GO(3); else LN_GO(4);
#undef LN_GO
}

extern "C" {

int tcl_conv1x1_small_f16(const void* x, int ldi, const void* W, const void* b, void* y, int ldo, long M, int Ci, int Co, hipStream_t st) {
    TCL_CHECK_ARG(x && W && b && y && Ci > 0 && Ci <= 8 && Ci <= ldi && Co > 0 && Co <= ldo && M > 0);
    hipLaunchKernelGGL(k_conv1x1_small, dim3(stream_grid(M, 256, 1)), dim3(256), 0, st, (const _Float16*)x, ldi, (const _Float16*)W, (const _Float16*)b,
                       (_Float16*)y, ldo, M, Ci, Co);
    TCL_LAUNCH_RET();
}
// workspace: per-block partials [B][nblk][64][2] f32, then the sums [B][64][2]
// The row partition of a sample depends on HW alone, never on the batch size: a sample's statistics are the same bits whether it is normalised alone
// or in a batch of 600 (unet.py relies on it: the identical CFG halves are computed once).  (Until round 3 the cap shrank with B.)
static inline int gn_blocks_cap(int B) { (void)B; return 256; }
size_t tcl_groupnorm_workspace_bytes(int B, int C) { (void)C; return ((size_t)B * gn_blocks_cap(B) + B) * 64 * 2 * 4 + 256; }
// k_gn_stats / k_gn_apply split an 8-channel chunk ONCE (head -> its first group, tail -> the group of its last channel): a chunk that starts
// `off` channels into a group and still reaches a third one (cpg - off channels of the first, cpg of the second, and some left: 2*cpg - off < 8) would
// be normalised with the wrong statistics.  The offsets 8k mod cpg repeat after cpg chunks at the latest.
static bool gn_chunk_spans_three_groups(int C, int cpg) {
    const int nchunk = C / 8;
    for (int k = 0; k < nchunk && k < cpg; ++k)
        if (2 * cpg - (8 * k) % cpg < 8) return true;
    return false;
}
int tcl_groupnorm_f16(const void* x1, int C1, const void* x2, int C2, const void* gamma, const void* beta, void* y, int B, int HW,
                      int groups, float eps, int silu, void* ws, hipStream_t st) {
    return tcl_groupnorm_concat_f16(x1, C1, x2, C2, gamma, beta, y, nullptr, B, HW, groups, eps, silu, ws, st);
}
int tcl_groupnorm_concat_f16(const void* x1, int C1, const void* x2, int C2, const void* gamma, const void* beta, void* y, void* yraw, int B, int HW,
                             int groups, float eps, int silu, void* ws, hipStream_t st) {
    const int C = C1 + C2;
    TCL_CHECK_ARG(x1 && gamma && beta && y && ws && B > 0 && HW > 0 && groups > 0 && groups <= 64 && C % groups == 0 && C / groups >= 4 && C1 % 8 == 0 && C2 % 8 == 0);
    TCL_CHECK_ARG(C2 == 0 || x2);
    TCL_CHECK_ARG(!gn_chunk_spans_three_groups(C, C / groups));
    int blocks = cdiv(HW, 64); if (blocks > gn_blocks_cap(B)) blocks = gn_blocks_cap(B);
    int rpb = cdiv(HW, blocks); blocks = cdiv(HW, rpb);
    float* part = (float*)ws; float* sums = part + (size_t)B * gn_blocks_cap(B) * 64 * 2;
    hipLaunchKernelGGL(k_gn_stats, dim3(blocks, B), dim3(256), 0, st, (const _Float16*)x1, C1, (const _Float16*)x2, C2, HW, groups, rpb, part);
    hipLaunchKernelGGL(k_gn_reduce, dim3(B), dim3(1024), 0, st, part, blocks, groups, sums);
    const int cwa = C / 8 < 256 ? C / 8 : 256, rpa = 256 / cwa;             // k_gn_apply: rows per block step; ~8 rows per thread, at most 2048 blocks per sample
    int gab = cdiv(HW, (long)rpa * 8); if (gab > 2048) gab = 2048;
#define GN_APPLY(S_, R_) hipLaunchKernelGGL((k_gn_apply<S_, R_>), dim3(gab, B), dim3(256), 0, st, \
                       (const _Float16*)x1, C1, (const _Float16*)x2, C2, sums, (const _Float16*)gamma, (const _Float16*)beta, \
                       1.f / ((float)HW * (float)(C / groups)), eps, groups, (_Float16*)y, HW, (_Float16*)yraw)
    if (silu) { if (yraw) GN_APPLY(true, true); else GN_APPLY(true, false); }
    else { if (yraw) GN_APPLY(false, true); else GN_APPLY(false, false); }
#undef GN_APPLY
    TCL_LAUNCH_RET();
}
int tcl_layernorm_f16(const void* x, const void* gamma, const void* beta, void* y, long rows, int C, float eps, hipStream_t st) {
    TCL_CHECK_ARG(x && gamma && beta && y && rows > 0 && C % 8 == 0 && C <= 2048);
    launch_layernorm<false>(x, gamma, beta, y, nullptr, rows, C, eps, st);
    TCL_LAUNCH_RET();
}
int tcl_layernorm_metric_f16(const void* x, const void* gamma, const void* beta, void* y, void* metric, long rows, int C, float eps, hipStream_t st) {
    TCL_CHECK_ARG(x && gamma && beta && y && metric && rows > 0 && C % 8 == 0 && C <= 2048);
    launch_layernorm<true>(x, gamma, beta, y, metric, rows, C, eps, st);
    TCL_LAUNCH_RET();
}
int tcl_geglu_f16(const void* in, void* out, long rows, int D, hipStream_t st) {
    TCL_CHECK_ARG(in && out && rows > 0 && D % 8 == 0);
    hipLaunchKernelGGL(k_geglu, dim3(stream_grid(rows * (D / 8), 256, 2)), dim3(256), 0, st, (const _Float16*)in, (_Float16*)out, rows, D);
    TCL_LAUNCH_RET();
}
int tcl_softmax_rows_f16(void* x, long rows, int T, int ld, float scale, hipStream_t st) {
    TCL_CHECK_ARG(x && rows > 0 && T > 0 && (size_t)T * 4 <= 150 * 1024);
    if (T % 8 == 0 && ld % 8 == 0 && T <= 16384) {
        hipLaunchKernelGGL(k_softmax_rows_reg, dim3((unsigned)rows), dim3(256), 0, st, (_Float16*)x, T, ld, scale);
        TCL_LAUNCH_RET();
    }
    static bool set = false;
    if (!set) { (void)hipFuncSetAttribute((const void*)k_softmax_rows, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024); set = true; }
    hipLaunchKernelGGL(k_softmax_rows, dim3((unsigned)rows), dim3(256), (size_t)T * 4, st, (_Float16*)x, T, ld, scale);
    TCL_LAUNCH_RET();
}
int tcl_concat_channels_f16(const void* x1, int C1, const void* x2, int C2, void* y, long rows, hipStream_t st) {
    TCL_CHECK_ARG(x1 && x2 && y && rows > 0 && C1 >= 0 && C2 >= 0 && C1 + C2 > 0 && C1 % 8 == 0 && C2 % 8 == 0);
    hipLaunchKernelGGL(k_concat, dim3(stream_grid(rows * ((C1 + C2) / 8), 256, 2)), dim3(256), 0, st, (const _Float16*)x1, C1, (const _Float16*)x2, C2, (_Float16*)y, rows);
    TCL_LAUNCH_RET();
}
int tcl_im2col3x3_small_f16(const void* x, void* out, int B, int H, int W, int Cin, int Kpad, hipStream_t st) {
    TCL_CHECK_ARG(x && out && B > 0 && H > 0 && W > 0 && Cin > 0 && Kpad >= 9 * Cin && Kpad % 64 == 0);
    hipLaunchKernelGGL(k_im2col_small, dim3(stream_grid((long)B * H * W * Kpad, 256, 4)), dim3(256), 0, st, (const _Float16*)x, (_Float16*)out, B, H, W, Cin, Kpad);
    TCL_LAUNCH_RET();
}
int tcl_gemv_f16(const void* W, const void* x, const void* bias, const void* add, void* y, int N, int K, int silu_in, int silu_out, hipStream_t st) {
    TCL_CHECK_ARG(W && x && y && K % 8 == 0);
    hipLaunchKernelGGL(k_gemv, dim3(cdiv(N, 4)), dim3(256), 0, st, (const _Float16*)W, (const _Float16*)x, (const _Float16*)bias, (const _Float16*)add,
                       (_Float16*)y, N, K, silu_in, silu_out);
    TCL_LAUNCH_RET();
}
int tcl_timestep_embed_f16(float t, int dim, void* out, hipStream_t st) {
    TCL_CHECK_ARG(out && dim % 2 == 0 && dim <= 2048);
    hipLaunchKernelGGL(k_timestep_embed, dim3(1), dim3(1024), 0, st, t, dim, (_Float16*)out);
    TCL_LAUNCH_RET();
}
int tcl_pack_latents_f16(const void* x, const void* cond, const int* idx, int F, int mode, int sl, int nwin, int h, int w, void* out, hipStream_t st) {
    TCL_CHECK_ARG(x && cond && idx && out && F > 0);
    long total = (long)F * (mode ? (long)nwin * h : (long)h * w);
    hipLaunchKernelGGL(k_pack_latents, dim3(stream_grid(total, 256, 1)), dim3(256), 0, st, (const _Float16*)x, (const _Float16*)cond, idx, F, mode, sl, nwin, h, w, (_Float16*)out);
    TCL_LAUNCH_RET();
}
int tcl_pack_latents12_f16(const void* x, const void* cond_fg, const void* cond_bg, int bg_frames, const int* idx, int F, int mode, int sl, int nwin,
                           int h, int w, void* out, hipStream_t st) {
    TCL_CHECK_ARG(x && cond_fg && cond_bg && idx && out && F > 0 && h > 0 && w > 0 && (mode == 0 || mode == 1) && ((uintptr_t)out & 7) == 0);
    TCL_CHECK_ARG(bg_frames >= 1);
    const int bg_one = bg_frames == 1;
    if (mode) {
        TCL_CHECK_ARG(sl >= 0 && nwin > 0);
        TCL_CHECK_ARG(bg_one || bg_frames >= sl + nwin);          // a per-frame background covers every frame the window reads
        const long tiles = (long)nwin * cdiv(F, PK12_T) * cdiv(h, PK12_T);
        hipLaunchKernelGGL(k_pack_latents12_yt, dim3((unsigned)(tiles > 8192 ? 8192 : tiles)), dim3(256), 0, st, (const _Float16*)x,
                           (const _Float16*)cond_fg, (const _Float16*)cond_bg, bg_one, idx, F, sl, nwin, h, w, (_Float16*)out);
    } else {
        hipLaunchKernelGGL(k_pack_latents12_xy, dim3(stream_grid((long)F * h * w, 256, 1)), dim3(256), 0, st, (const _Float16*)x,
                           (const _Float16*)cond_fg, (const _Float16*)cond_bg, bg_one, idx, F, h, w, (_Float16*)out);
    }
    TCL_LAUNCH_RET();
}
int tcl_unpack_cfg_f16(const void* eps, const int* idx, int F, int mode, int sl, int nwin, int h, int w, float guidance, int scale_upto,
                       float scale, int nkeep, void* noise, hipStream_t st) {
    TCL_CHECK_ARG(eps && idx && noise && F > 0);
    long total = (long)F * (mode ? (long)nwin * h : (long)h * w);
    hipLaunchKernelGGL(k_unpack_cfg, dim3(stream_grid(total, 256, 1)), dim3(256), 0, st, (const _Float16*)eps, idx, F, mode, sl, nwin, h, w, guidance, scale_upto, scale, nkeep, (_Float16*)noise);
    TCL_LAUNCH_RET();
}
int tcl_adain_fuse_f16(void* noises_t, void* noises, int planes, int hw, float alpha, hipStream_t st) {
    TCL_CHECK_ARG(noises_t && noises && planes > 0 && hw > 1);
    hipLaunchKernelGGL(k_adain_fuse, dim3(planes), dim3(256), 0, st, (_Float16*)noises_t, (_Float16*)noises, hw, alpha);
    TCL_LAUNCH_RET();
}
int tcl_dpm_sde_step_f16(void* x, const void* eps, float* m0, const float* m1, const void* z, long n, float sigma_t, float alpha_t, float ca,
                         float cb0, float cb1, float cc, hipStream_t st) {
    TCL_CHECK_ARG(x && eps && m0 && n > 0);
    hipLaunchKernelGGL(k_dpm_step, dim3(stream_grid(n, 256, 2)), dim3(256), 0, st, (_Float16*)x, (const _Float16*)eps, m0, m1, (const _Float16*)z, n, sigma_t, alpha_t, ca, cb0, cb1, cc);
    TCL_LAUNCH_RET();
}
int tcl_invert_pack_f16(const float* x, const void* cond, const int* idx, int N, int F, int h, int w, void* out, hipStream_t st) {
    TCL_CHECK_ARG(x && cond && idx && out && N > 0 && F > 0 && h > 0 && w > 0);
    const long hw = (long)h * w;
    hipLaunchKernelGGL(k_invert_pack, dim3(stream_grid((long)F * hw, 256, 1)), dim3(256), 0, st, x, (const _Float16*)cond, idx, N, F, hw, (_Float16*)out);
    TCL_LAUNCH_RET();
}
int tcl_ddim_step_f32(float* x, const void* eps, const int* idx, int N, int F, int F_valid, int h, int w, float mu, float sigma, float mu_prev,
                      float sigma_prev, int inversion, void* xin, hipStream_t st) {
    TCL_CHECK_ARG(x && eps && idx && xin && N > 0 && F > 0 && F_valid > 0 && F_valid <= F && h > 0 && w > 0 && mu > 0.f && mu_prev > 0.f);
    const long hw = (long)h * w;
    // (a, b) = (prev, t) stepping up the noise levels, (t, prev) stepping down
    const float s_a = inversion ? sigma_prev : sigma, m_a = inversion ? mu_prev : mu, m_b = inversion ? mu : mu_prev, s_b = inversion ? sigma : sigma_prev;
    hipLaunchKernelGGL(k_ddim_step, dim3(stream_grid((long)F_valid * hw, 256, 1)), dim3(256), 0, st, x, (const _Float16*)eps, idx, N, F_valid, hw,
                       s_a, m_a, m_b, s_b, (_Float16*)xin);
    TCL_LAUNCH_RET();
}
int tcl_img_to_nhwc8_f16(const float* img, void* out, int B, int HW, hipStream_t st) {
    TCL_CHECK_ARG(img && out && B > 0 && HW > 0);
    hipLaunchKernelGGL(k_img_to_nhwc, dim3(stream_grid((long)B * HW, 256, 1)), dim3(256), 0, st, img, (_Float16*)out, B, HW);
    TCL_LAUNCH_RET();
}
int tcl_nhwc_to_img_f32(const void* y, int ldc, float* img, int B, int HW, hipStream_t st) {
    TCL_CHECK_ARG(y && img && B > 0 && HW > 0 && ldc >= 3);
    hipLaunchKernelGGL(k_nhwc_to_img, dim3(stream_grid((long)B * HW, 256, 1)), dim3(256), 0, st, (const _Float16*)y, ldc, img, B, HW);
    TCL_LAUNCH_RET();
}
int tcl_nhwc_to_nchw_f16(const void* y, int ldc, void* out, int B, int C, int HW, float scale, hipStream_t st) {
    TCL_CHECK_ARG(y && out && B > 0 && HW > 0 && C > 0 && ldc >= C);
    hipLaunchKernelGGL(k_nhwc_to_nchw, dim3(stream_grid((long)B * HW, 256, 1)), dim3(256), 0, st, (const _Float16*)y, ldc, (_Float16*)out, B, C, HW, scale);
    TCL_LAUNCH_RET();
}
int tcl_nchw_to_nhwc_f16(const void* x, void* out, int ldc, int B, int C, int HW, float scale, hipStream_t st) {
    TCL_CHECK_ARG(x && out && B > 0 && HW > 0 && C > 0 && ldc >= C);
    hipLaunchKernelGGL(k_nchw_to_nhwc, dim3(stream_grid((long)B * HW, 256, 1)), dim3(256), 0, st, (const _Float16*)x, (_Float16*)out, ldc, B, C, HW, scale);
    TCL_LAUNCH_RET();
}
int tcl_transpose_f16(const void* in, void* out, int batch, int R, int Cc, int ldi, int ldo, hipStream_t st) {
    TCL_CHECK_ARG(in && out && batch > 0 && R > 0 && Cc > 0 && ldi >= Cc && ldo >= R);
    hipLaunchKernelGGL(k_transpose, dim3(cdiv(Cc, 32), cdiv(R, 32), batch), dim3(32, 8), 0, st, (const _Float16*)in, (_Float16*)out, R, Cc, ldi, ldo);
    TCL_LAUNCH_RET();
}

}  // extern "C"
