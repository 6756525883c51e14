// Flash attention forward for gfx950 (f16 in, f32 softmax/accumulate), head_dim 40 / 80 / 160 (SD-1.5 UNet) --
// the self-attention over VidToMe-merged tokens (T up to ~47k) and the text cross-attention that the reference runs
// through torch SDPA / xformers (AttnProcessor2_0, utils/model_utils.py:66-67; patch.py:170-176).  T x T scores are
// never materialised.
//
// What is in this file:
//  pack : Q,K,V rows (heads interleaved in channels) -> head-major, zero-padded panels, one launch (k_pack_qkv; k_pack_rows / k_pack_vt when only
//           a part is packed): Qp [B,H,Tqp,DP] (pre-scaled by softmax_scale*log2 e), Kp [B,H,Tkp,DP+8], Vt [B,H,Tkp/64,DPV,V_STRIDE] (V transposed and
//           tile-major, so that a 64-key K or V^T tile is one contiguous LDS image).  DP = d rounded to 16, DPV = d rounded to 32.
//  flash: k_flash, block = 4 waves x QB blocks of 32 query rows.  64-key K / V^T tiles go global -> LDS by LDS-DMA (global_load_lds_dwordx4,
//           no VGPR staging) into a ring of NSTG slots, prefetch distance NSTG - 1, counted vmcnt and one raw barrier per tile -- or per pair
//           of tiles (TPB = 2, 4-slot ring).  S^T = K.Q^T with mfma_f32_32x32x16_f16 (swapped operands: lane l owns query l&31, so the row
//           max/sum is in-lane + one lane<->lane+32 exchange); P stays in registers as the B operand of O^T = V^T.P^T (the key permutation
//           of the accumulator layout is matched by the V^T fragment addresses instead of shuffling P).  Block id -> head = id % H so that
//           each head's K/V panel lives in one XCD's L2.  The forms choose() picks from: the rows of g_flash.
//  split-KV: k_flash_lse (the d = 128 body over one chunk of the keys per batch entry, which also hands on log2 of its softmax denominator)
//           and k_attn_merge (joins the chunks' partial outputs).
#include "common.h"
#include "gemm_conv.h"
#include "prof.h"
#include "../../include/tclight_hip.h"
#include <stdlib.h>
#include <type_traits>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float float16v __attribute__((ext_vector_type(16)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// one_col >= 0: that column (a padding column, >= d) is set to 1 in valid rows (the K panel's ones column for the folded shift)
__device__ __forceinline__ void pack_rows_blk(int blk, int nblk, const _Float16* __restrict__ src, long bstride, int ld, int T, int H, int d, float scale,
                                              _Float16* __restrict__ dst, int Tp, int DP, long total_chunks, int one_col) {
    const int cpr = DP / 8;
    for (long i = (long)blk * blockDim.x + threadIdx.x; i < total_chunks; i += (long)nblk * blockDim.x) {
        int c8 = (int)(i % cpr) * 8; long row = i / cpr; int t = (int)(row % Tp); long bh = row / Tp; int h = (int)(bh % H); long b = bh / H;
        half8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;
        if (t < T && c8 < d) {
            v = *(const half8*)(src + b * bstride + (long)t * ld + h * d + c8);
            if (scale != 1.f)
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (_Float16)((float)v[j] * scale);
        }
        if (t < T && one_col >= c8 && one_col < c8 + 8) v[one_col - c8] = (_Float16)1.f;
        *(half8*)(dst + i * 8) = v;
    }
}
__global__ void k_pack_rows(const _Float16* __restrict__ src, long bstride, int ld, int T, int H, int d, float scale,
                            _Float16* __restrict__ dst, int Tp, int DP, long total_chunks, int one_col) {
    pack_rows_blk(blockIdx.x, gridDim.x, src, bstride, ld, T, H, d, scale, dst, Tp, DP, total_chunks, one_col);
}
// Vt panel, tile-major: Vt[bh][tile][i][p(t)] = V[b][tile*64 + t][h*d + i], rows of V_STRIDE halves (64 keys + pad), so that one
// 64-key tile is a contiguous LDS image (DPV x V_STRIDE).  Within every group of 16 keys the two middle blocks of 4 are swapped
// (p swaps bits 2 and 3 of t): the S^T accumulator of the flash kernel leaves lane half hl with keys {4hl..4hl+3, 8+4hl..8+4hl+3}
// of a group, and with this order those 8 V^T values are one contiguous 16-B LDS read (8*hl .. 8*hl+7).  Row D (when DPV > D) is
// a row of ones over the valid keys: the PV MFMA then also yields the softmax row sums.
// skew (head_dim 40, whose PV runs on 16x16x32 MFMAs): rows 4..11 (mod 16) swap the two 16-key halves of every 32-key block (position ^ 16).
// The 16x16x32 A fragment read has lane l fetch row l & 15 at key group l >> 4, and a ds_read_b128 lane group mixes rows 0-3 / 12-15 of one
// key group with rows 4-11 of another: without the skew two pairs of lanes share a 16-B bank slot (SQ_LDS_BANK_CONFLICT = 1/3 of the kernel's
// LDS cycles); with it all 16 slots of the 256-B bank window are distinct (exhaustive check of the four lane groups).
__device__ __forceinline__ void pack_vt_blk(int tile_idx, int bh, const _Float16* __restrict__ v, long bstride, int ld, int T, int H, int d,
                                            _Float16* __restrict__ vt, int ntiles, int DPV, int skew) {
    extern __shared__ _Float16 tile[];   // [64][DPV+2]
    const int t0 = tile_idx * 64, h = bh % H; const long b = bh / H;
    const int st = DPV + 2, cpr = DPV / 8;
    for (int i = threadIdx.x; i < 64 * cpr; i += 256) {
        int r = i / cpr, c8 = (i % cpr) * 8, t = t0 + r;
        half8 x;
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (_Float16)0.f;
        if (t < T && c8 < d) x = *(const half8*)(v + b * bstride + (long)t * ld + h * d + c8);
#pragma unroll
        for (int j = 0; j < 8; ++j) tile[r * st + c8 + j] = x[j];
    }
    __syncthreads();
    _Float16* out = vt + ((long)bh * ntiles + tile_idx) * vt_tile_halves(DPV);
    for (int i = threadIdx.x; i < DPV * 64; i += 256) {
        int dd = i / 64, r = i % 64;
        _Float16 val = tile[r * st + dd];
        if (dd == d && DPV > d) val = (t0 + r < T) ? (_Float16)1.f : (_Float16)0.f;
        int pr = (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1);
        if (skew && (((dd & 15) + 4) & 8)) pr ^= 16;
        out[dd * V_STRIDE + pr] = val;
    }
}
__global__ __launch_bounds__(256) void k_pack_vt(const _Float16* __restrict__ v, long bstride, int ld, int T, int H, int d,
                                                 _Float16* __restrict__ vt, int ntiles, int DPV, int skew) {
    pack_vt_blk(blockIdx.x, blockIdx.y, v, bstride, ld, T, H, d, vt, ntiles, DPV, skew);
}
// Q, K and V^T panels of one attention call in ONE launch (round 4: they were three -- 170 k launches of ~28 us per 300-frame pass on the main
// stream): blocks [0, gq) pack Q rows, [gq, gq + gk) K rows, the rest one V^T tile each.  Same device functions, same bits.
struct PackRows { const _Float16* src; long bstride; int ld, T, d; float scale; _Float16* dst; int Tp, DP; long total; int one_col; };
__global__ __launch_bounds__(256) void k_pack_qkv(PackRows q, PackRows k, int gq, int gk, int H, const _Float16* __restrict__ v, long vbs, int ldv, int Tk, int d,
                                                  _Float16* __restrict__ vt, int ntiles, int DPV, int skew) {
    const int blk = blockIdx.x;
    if (blk < gq) pack_rows_blk(blk, gq, q.src, q.bstride, q.ld, q.T, H, q.d, q.scale, q.dst, q.Tp, q.DP, q.total, q.one_col);
    else if (blk < gq + gk) pack_rows_blk(blk - gq, gk, k.src, k.bstride, k.ld, k.T, H, k.d, k.scale, k.dst, k.Tp, k.DP, k.total, k.one_col);
    else { const int i = blk - gq - gk; pack_vt_blk(i % ntiles, i / ntiles, v, vbs, ldv, Tk, H, d, vt, ntiles, DPV, skew); }
}

// Flash kernel.  Block = 4 waves; each wave owns QB blocks of 32 queries (QB = 2 for head_dim 40: the K and V^T fragments read
// from LDS feed two MFMAs each, which halves the LDS traffic per MFMA -- measured as the co-bottleneck of the one-block version).
// K/V tiles (64 keys) are contiguous "LDS images" in the panels (K rows padded to KS = DP + 8 halves, V^T rows to V_STRIDE), so
// staging is pure LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave instruction, no VGPR staging, no ds_write): ring of NSTG slots,
// prefetch distance NSTG - 1, counted vmcnt + one raw barrier per tile (a __syncthreads() would drain the DMA queue).
// Per tile and query block: S^T = K.Q^T (swapped operands: lane l owns query l&31, so row max/sum are in-lane + one exchange
// with lane l+32), online softmax with lazy rescale (only when some running max grows by more than 2^6), P stays in registers
// as the B operand of O^T += V^T.P^T; row sums come out of the same MFMA through the ones-row of the V^T panel.
// filler source for the DMA pieces behind a stage's end: every lane reads 16 B at lane * 16, so it must span a whole 1 KiB piece (a 256-B
// array let lanes 16-63 read past it -- whatever followed in the code object's data segment, or a fault when that was the segment's end)
__device__ __attribute__((aligned(1024))) unsigned g_flash_zero[256];

// max over the two 32-lane halves without the LDS round trip of a shuffle: v_permlane32_swap exchanges a's upper half with b's lower half
__device__ __forceinline__ float xhalf_max(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// (the body of k_flash for ONE block index: the kernel below calls it once, or -- the flag-gated exact pass behind the speculative kernel -- once per
// flagged index of its stride class)
// KVI: the K / V panel of sample b is kv_index[b] (a per-block scalar load: b is uniform over the block) instead of b / kv_div -- the per-frame text of
// generation.prompt_path.  Instantiated beside the kernels without it, whose code is what it was.
template <int D, int DP, int DPV, int QB, int NSTG, int TPB, int MINB, int SPEC, bool SPLIT = false, bool KVI = false>
__device__ __forceinline__ void flash_block(const int bid, const _Float16* __restrict__ Qp, const _Float16* __restrict__ Kp, const _Float16* __restrict__ Vt,
                                            _Float16* __restrict__ O, int H, int Tq, int Tk, int Tqp, int Tkp, int d, int ldo, long obstride,
                                            int kv_div, int nqb, int* __restrict__ flags, float* __restrict__ lse = nullptr,
                                            const int* __restrict__ kv_index = nullptr) {
    constexpr int KS = DP + 8;                    // K row stride (halves); KS/8 odd -> conflict-free b128 reads
    constexpr int NQK = DP / 16, NDT = DPV / 32;
    constexpr int KBYTES = KV_TILE * KS * 2, VBYTES = vt_tile_halves(DPV) * 2, SBYTES = KBYTES + VBYTES;
    // 1-KiB DMA pieces of a stage, and pieces per wave (4 waves per block: a K / V^T stage serves 128 QB queries)
    constexpr int NPIECE = (SBYTES + 1023) / 1024, NPW = (NPIECE + 3) / 4, SSTRIDE = NPIECE * 1024;
    constexpr bool LROW = DPV > D;
    constexpr bool FOLD = DP > D && LROW && (D % 16 == 8);        // spare Q/K column D: lanes hl == 1, element 0 of fragment D/16
    constexpr bool PVQ = QB > 1;                                  // PV per query block right behind its softmax (V^T fragments held in registers)
    // PV16 (head_dim 40): O^T = V^T.P^T on 16x16x32 MFMAs over 48 V^T rows (40 + the ones row + 7 idle) instead of 32x32x16 over 64: 12
    // MFMAs of 16 cycles per query block and tile instead of 8 of 32 (-25 % PV matrix time).  The 32x32 S^T accumulator leaves lane l with
    // query l & 31; a 16x16x32 B operand wants query l & 15 in all four 16-lane rows, the rows being four 8-key groups.  One
    // v_permlane16_swap per register pair (first-8-keys register X, second-8-keys register Y of a 32-key block) does exactly that exchange:
    // X.row1 <-> Y.row0, X.row3 <-> Y.row2 turns X into the operand of queries 0-15 and Y into that of queries 16-31, key groups in the order
    // (A, B, C, D) = keys {0-3,8-11}, {16-19,24-27}, {4-7,12-15}, {20-23,28-31} -- which the V^T panel's in-tile key permutation already
    // stores at halves 0, 16, 8, 24 of a 32-key block.
    constexpr bool PV16 = D == 40 && LROW && DPV >= 48;
    constexpr int NT16 = 3;                                       // 16-row V^T tiles: rows 0-39 V, row 40 ones, 41-47 zero
    extern __shared__ __attribute__((aligned(16))) char smem[];          // 3 stages of SSTRIDE bytes + 1 KiB dump

    const int head = bid % H, qb_ = (bid / H) % nqb, b = bid / (H * nqb);
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), hl = lane >> 5, ql = lane & 31;
    const int q0 = qb_ * (128 * QB) + wid * (32 * QB);
    const long bh = (long)b * H + head, kbh = (long)(KVI ? kv_index[b] : b / kv_div) * H + head;
    const int nt = Tkp / KV_TILE, nfull = Tk / KV_TILE;      // tiles / tiles without padded keys
    const char* kbase = (const char*)(Kp + kbh * Tkp * KS);
    const char* vbase = (const char*)(Vt + kbh * nt * vt_tile_halves(DPV));
    const char* zero = (const char*)g_flash_zero;

    half8 qf[QB][NQK];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const _Float16* qrow = Qp + (bh * Tqp + q0 + qb * 32 + ql) * DP + 8 * hl;
#pragma unroll
        for (int ks = 0; ks < NQK; ++ks) qf[qb][ks] = *(const half8*)(qrow + ks * 16);
    }
    // DMA: piece p = wid + 4 i covers stage bytes [1024 p, 1024 p + 1024); K image first, V^T image behind it.  The piece index is
    // wave-uniform and the K / V^T boundary is piece-aligned (KBYTES = 128 KS, 8 | KS), so a piece's source is a SCALAR base (s_cselect
    // between the two panels) plus the one per-lane offset lane * 16 -- no per-lane selects, no per-piece address registers (an earlier
    // version spent 76 vector instructions per pair of tiles on those selects; a per-piece pointer table spilled the d >= 80 kernels).
    // Only a V^T image that is not a multiple of 1 KiB (DPV = 96) needs the per-lane zero filler behind its end.
    static_assert(KBYTES % 1024 == 0, "K image must be piece-aligned");
    const int lane16 = lane * 16;
    __attribute__((address_space(3))) char* const lds0 = (__attribute__((address_space(3))) char*)smem;
#define FLASH_ISSUE(IT)                                                                                                       \
    {                                                                                                                         \
        const char* kt_ = kbase + (long)(IT) * KBYTES;                                                                        \
        const char* vt_ = vbase + (long)(IT) * VBYTES;                                                                        \
        const int st_ = ((IT) % NSTG) * SSTRIDE;                                                                              \
        _Pragma("unroll") for (int i = 0; i < NPW; ++i) {                                                                    \
            const int pb_ = (wid + 4 * i) * 1024;                                                                            \
            const char* src_ = (pb_ < KBYTES ? kt_ + pb_ : vt_ + (pb_ - KBYTES)) + lane16;                                    \
            if (SBYTES % 1024 != 0) src_ = pb_ + lane16 < SBYTES ? src_ : zero + lane16;                                      \
            else if (NSTG != 3 && NPW * 4 != NPIECE && (wid + 4 * i) >= NPIECE) continue;   /* nothing to issue past the stage (wave-uniform; the 3-slot ring COUNTS its pieces: it keeps the dump piece) */ \
            const int dst_ = (wid + 4 * i) < NPIECE ? st_ + pb_ : NSTG * SSTRIDE;      /* pieces past the stage: 1 KiB dump */  \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src_,                             \
                                             (__attribute__((address_space(3))) void*)(lds0 + dst_), 16, 0, 0);               \
        }                                                                                                                     \
    }

    float16v o[QB][PV16 ? 1 : NDT];
    float4v o16[QB][2][PV16 ? NT16 : 1];          // PV16: [query block][queries 0-15 | 16-31][16-row tile]; lane l: rows 4 (l >> 4) + r, query l & 15
    float m[QB], lsum[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        m[qb] = FOLD ? 0.f : -1e30f; lsum[qb] = 0.f;
#pragma unroll
        for (int t = 0; t < (PV16 ? 1 : NDT); ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[qb][t][r] = 0.f;
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int t = 0; t < (PV16 ? NT16 : 1); ++t) o16[qb][qt][t] = float4v{0.f, 0.f, 0.f, 0.f};
    }

    // MK = std::true_type: the tile may hold padded keys (only the last one does).  A compile-time switch, not `if (it >= nfull)`: hipcc turns
    // that runtime test into 126 unconditional v_cmp / v_cndmask / v_add per tile -- half of this VALU-bound loop's vector instructions.
    // SPEC (head_dim 40): the loop is bound by vector ISSUE (tools/micro/flash_mix.hip: its instruction mix allows the matrix pipe 52 % with
    // the row maxima, 62 % without), and the row maximum is the one term that only guards the f16 range of P.  So the shift m is kept OFF = 3
    // bits ABOVE the running row maximum (P <= 2^-3 in the common case; weights below 2^-21 of the row maximum vanish where the textbook P <= 1
    // keeps them down to 2^-24: measured on rows with a sink key 20 bits above the rest, 3.0e-4 rel-L2 against 2.2e-4 for the exact kernel (5.5e-4 with OFF = 4),
    // tests/test_gpu_fullsize.py::test_attention_heavy_tail_and_sink_precision), P is computed without looking at the scores, and the guard reads
    // the result: OR of the packed P registers, bit 14 of a half set <=> some P >= 2 <=> a score rose 4 bits above the maximum the shift was
    // made for.  The guard is evaluated AFTER the tile's PV MFMAs are issued (P in [2, 65504] is still exact, so that PV was right): then
    // `rebase` recomputes the tile's scores from the K tile still in LDS, takes the exact row maxima and moves shift, Q column and O.
    // What this cannot catch in time is a P beyond the f16 range (a score 19 bits above everything the row had seen, inside one tile): the
    // row sum then comes out inf / NaN, the block flags itself and the launch that follows (the exact-maximum kernel, gated by the flags)
    // redoes that block.  Tile 0 starts with a rebase (there is no shift yet).  Scores that keep climbing along the key sequence make every
    // tile pair pay a rebase (keys scaled by a ramp 0.3 .. 6 along the sequence: 567 against 758 TFLOP/s for the exact kernel); keys in
    // token order have no such trend.  Tiles with padded keys (the last one) take the exact-maximum
    // path below -- same shift convention, any shift is valid there -- so the speculative code carries no key masks.
    constexpr float OFF = 3.f;
    unsigned orv = 0;                                 // SPEC: OR of the packed P registers since the last guard test
    static_assert(!SPEC || (FOLD && (PV16 || PVQ)), "the speculative softmax is the head_dim-40 path");
    auto rebase = [&](const int it, const bool first) __attribute__((always_inline)) {
        if constexpr (SPEC) {
        const _Float16* kt = (const _Float16*)(smem + (it % NSTG) * SSTRIDE);
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            float16v s[2];
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[blk][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < NQK; ++ks)
                    s[blk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const half8*)(kt + (blk * 32 + ql) * KS + 8 * hl + ks * 16), qf[qb][ks], s[blk], 0, 0, 0);
            }
            float mx = -1e30f;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[blk][r]);
            mx = xhalf_max(mx) + OFF;                                            // (scores are relative to the current shift)
            const float mn = (float)(_Float16)(m[qb] + (first ? mx : fmaxf(mx, 0.f)));      // the shift only ever grows; kept f16-representable
            const float delta = mn - m[qb], alpha = __builtin_amdgcn_exp2f(-delta);
            m[qb] = mn;
            if (hl == 1) qf[qb][D / 16][0] = (_Float16)(-mn);                    // Q[q][D] lives in fragment D/16, lanes hl == 1, element 0
            if (!first) {
                if constexpr (PV16) {
#pragma unroll
                    for (int qt = 0; qt < 2; ++qt) {
                        const float aq = __shfl(alpha, (lane & 15) + 16 * qt, 64);   // this accumulator's query sits in another lane of the S^T layout
#pragma unroll
                        for (int t = 0; t < NT16; ++t) o16[qb][qt][t] *= aq;
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < NDT; ++t)
#pragma unroll
                        for (int r = 0; r < 16; ++r) o[qb][t][r] *= alpha;           // 32x32 O^T: the query is this lane's own
                }
            }
        }
        }
    };
    auto tile = [&](const int it, auto MK) __attribute__((always_inline)) {
        const _Float16* kt = (const _Float16*)(smem + (it % NSTG) * SSTRIDE);
        const _Float16* vt = kt + KV_TILE * KS;
        constexpr bool mask = decltype(MK)::value;
        half8 kf[2][NQK];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int ks = 0; ks < NQK; ++ks) kf[blk][ks] = *(const half8*)(kt + (blk * 32 + ql) * KS + 8 * hl + ks * 16);
        half8 pf[QB][2][2];
        half8 vfr[PVQ && !PV16 ? 2 : 1][2][NDT];     // PVQ: every V^T fragment of the tile in registers (read once, early)
        half8 vf16[PV16 ? 2 : 1][NT16];               // PV16: row t 16 + (l & 15), the 8 keys of group l >> 4 of 32-key block blk
        if constexpr (PV16) {
            const int goff = (((lane >> 4) & 1) * 16 + (lane >> 5) * 8) ^ ((((lane & 15) + 4) & 8) ? 16 : 0);      // (^ 16: the panel's row skew, k_pack_vt)
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int t = 0; t < NT16; ++t) vf16[blk][t] = *(const half8*)(vt + (t * 16 + (lane & 15)) * V_STRIDE + blk * 32 + goff);
        } else if constexpr (PVQ) {
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int ss = 0; ss < 2; ++ss)
#pragma unroll
                    for (int t = 0; t < NDT; ++t) vfr[blk][ss][t] = *(const half8*)(vt + (ql + t * 32) * V_STRIDE + blk * 32 + 16 * ss + 8 * hl);
        }
        // all QK^T MFMAs of the tile first (QB * 2 * NQK back to back): the row-maximum VALU work of query block 0 then runs under the
        // MFMAs of query block 1 still in the pipe, instead of each block's maximum waiting for its own MFMAs with the pipe idle
        float16v sacc[QB][2];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[qb][blk][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < NQK; ++ks) sacc[qb][blk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[blk][ks], qf[qb][ks], sacc[qb][blk], 0, 0, 0);
            }
        if constexpr (mask) {
#pragma unroll
            for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { int kv = it * KV_TILE + blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl; if (kv >= Tk) sacc[qb][blk][r] = -1e30f; }
        }
        if constexpr (SPEC && !mask) {
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                float16v (&s)[2] = sacc[qb];
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) pf[qb][blk][r >> 3][r & 7] = (_Float16)__builtin_amdgcn_exp2f(s[blk][r]);
                    u32x4 x = __builtin_bit_cast(u32x4, pf[qb][blk][0]), y = __builtin_bit_cast(u32x4, pf[qb][blk][1]);
                    orv |= x[0] | x[1] | x[2] | x[3] | y[0] | y[1] | y[2] | y[3];
                    if constexpr (PV16) {
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            const auto sw = __builtin_amdgcn_permlane16_swap(x[w], y[w], false, false);
                            x[w] = sw[0]; y[w] = sw[1];
                        }
                        const half8 p0 = __builtin_bit_cast(half8, x), p1 = __builtin_bit_cast(half8, y);      // queries 0-15 | 16-31
#pragma unroll
                        for (int t = 0; t < NT16; ++t) {
                            o16[qb][0][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf16[blk][t], p0, o16[qb][0][t], 0, 0, 0);
                            o16[qb][1][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf16[blk][t], p1, o16[qb][1][t], 0, 0, 0);
                        }
                    } else {
#pragma unroll
                        for (int ss = 0; ss < 2; ++ss)
#pragma unroll
                            for (int t = 0; t < NDT; ++t) o[qb][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vfr[blk][ss][t], pf[qb][blk][ss], o[qb][t], 0, 0, 0);
                    }
                }
            }
            if constexpr (TPB == 1) {
                if (__any((orv & 0x40004000u) != 0u)) {
                    asm volatile("; rebase");                                   // keeps this rare path a real branch
                    rebase(it, false);
                }
                orv = 0;
            }
            return;
        }
        // row maxima of every query block first, then ONE (rare) branch for all re-basing of the tile, so that the common path below --
        // exponentials, conversions and the PV MFMAs of all query blocks -- is a single basic block the scheduler can interleave
        float mxq[QB];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            float mx = sacc[qb][0][0];
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[qb][blk][r]);
            mxq[qb] = xhalf_max(mx);
        }
        bool need = it == 0;
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) need |= FOLD ? (mxq[qb] > 6.f) : (mxq[qb] > m[qb] + 6.f);
        if (__any(need)) {
            asm volatile("; rebase");       // keeps this rare path a real branch (hipcc otherwise runs the multiplies and
                                                         // subtractions below on every tile with alpha = 1 / delta = 0 selected in)
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                float16v (&s)[2] = sacc[qb];
                const float mx = mxq[qb];
                if constexpr (FOLD) {
                    // The running shift m (kept f16-representable) rides in the spare Q column D against a ones column of the K panel, so
                    // the MFMA already returned s - m and the common path is exp2 alone.  Any shift works as long as every key of the row
                    // uses the same one between rescales; it is re-based when the row maximum climbs more than 2^6 above it (and on tile 0).
                    if (it == 0 || __any(mx > 6.f)) {
                        const float mn = (float)(_Float16)(m[qb] + (it == 0 ? mx : fmaxf(mx, 0.f)));
                        const float delta = mn - m[qb], alpha = __builtin_amdgcn_exp2f(-delta);
                        m[qb] = mn;
                        if (hl == 1) qf[qb][D / 16][0] = (_Float16)(-mn);        // Q[q][D] lives in fragment D/16, lanes hl == 1, element 0
                        if constexpr (PV16) {
#pragma unroll
                            for (int qt = 0; qt < 2; ++qt) {
                                const float aq = __shfl(alpha, (lane & 15) + 16 * qt, 64);      // this accumulator's query sits in another lane of the S^T layout
#pragma unroll
                                for (int t = 0; t < NT16; ++t) o16[qb][qt][t] *= aq;
                            }
                        } else {
#pragma unroll
                            for (int t = 0; t < NDT; ++t)
#pragma unroll
                                for (int r = 0; r < 16; ++r) o[qb][t][r] *= alpha;
                        }
#pragma unroll
                        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                            for (int r = 0; r < 16; ++r) s[blk][r] -= delta;
                    }
                } else if (__any(mx > m[qb] + 6.f)) {          // lazy rescale (rare after the first tiles)
                    const float mn = fmaxf(m[qb], mx), alpha = __builtin_amdgcn_exp2f(m[qb] - mn);
                    m[qb] = mn;
                    lsum[qb] *= alpha;
#pragma unroll
                    for (int t = 0; t < NDT; ++t)
#pragma unroll
                        for (int r = 0; r < 16; ++r) o[qb][t][r] *= alpha;
                }
            }
        }
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            float16v (&s)[2] = sacc[qb];
            float ps = 0.f;
            if (FOLD) {
#pragma unroll
                for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                    for (int r = 0; r < 16; ++r) pf[qb][blk][r >> 3][r & 7] = (_Float16)__builtin_amdgcn_exp2f(s[blk][r]);
            } else {
#pragma unroll
                for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { float p = __builtin_amdgcn_exp2f(s[blk][r] - m[qb]); if (!LROW) ps += p; pf[qb][blk][r >> 3][r & 7] = (_Float16)p; }
            }
            if (!LROW) lsum[qb] += ps;
            if constexpr (PV16) {
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    u32x4 x = __builtin_bit_cast(u32x4, pf[qb][blk][0]), y = __builtin_bit_cast(u32x4, pf[qb][blk][1]);
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const auto sw = __builtin_amdgcn_permlane16_swap(x[w], y[w], false, false);
                        x[w] = sw[0]; y[w] = sw[1];
                    }
                    const half8 p0 = __builtin_bit_cast(half8, x), p1 = __builtin_bit_cast(half8, y);      // queries 0-15 | 16-31
#pragma unroll
                    for (int t = 0; t < NT16; ++t) {
                        o16[qb][0][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf16[blk][t], p0, o16[qb][0][t], 0, 0, 0);
                        o16[qb][1][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf16[blk][t], p1, o16[qb][1][t], 0, 0, 0);
                    }
                }
            } else if constexpr (PVQ) {
                // this query block's PV right behind its softmax: the 4 * NDT MFMAs run while the NEXT block's exponentials issue on the
                // vector pipe (one wave then overlaps its own matrix and vector work instead of leaving that to its SIMD partner)
#pragma unroll
                for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                    for (int ss = 0; ss < 2; ++ss)
#pragma unroll
                        for (int t = 0; t < NDT; ++t) o[qb][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vfr[blk][ss][t], pf[qb][blk][ss], o[qb][t], 0, 0, 0);
            }
        }
        if constexpr (!PVQ && !PV16) {
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int ss = 0; ss < 2; ++ss) {
                    const _Float16* vr = vt + ql * V_STRIDE + blk * 32 + 16 * ss + 8 * hl;
#pragma unroll
                    for (int t = 0; t < NDT; ++t) {
                        const half8 vf = *(const half8*)(vr + t * 32 * V_STRIDE);
#pragma unroll
                        for (int qb = 0; qb < QB; ++qb) o[qb][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[qb][blk][ss], o[qb][t], 0, 0, 0);
                    }
                }
        }
    };
    if constexpr (TPB == 2) {
        // 4-slot ring, two tiles per barrier: tiles it, it+1 are consumed while it+2, it+3 stream into the slots of it-2, it-1 --
        // half the rendezvous of the one-tile loop (the waves of a block sit on four SIMDs with different partners and drift apart)
        static_assert(NSTG == 4, "two tiles per barrier need a 4-slot ring");
        FLASH_ISSUE(0);
        if (nt > 1) FLASH_ISSUE(1);
        int it = 0;
        for (; it + 1 < nfull; it += 2) {             // pairs of tiles without padded keys: the hot loop
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();             // tiles it, it+1 landed for every wave; everyone is done with it-2, it-1
            if (it + 2 < nt) FLASH_ISSUE(it + 2);
            if (it + 3 < nt) FLASH_ISSUE(it + 3);
            if (SPEC && it == 0) rebase(0, true);
            tile(it, std::false_type{});
            tile(it + 1, std::false_type{});
            if constexpr (SPEC) {
                // ONE guard test per pair of tiles, behind both tiles' work (the OR result is long there: no stall on it, and the pair is one
                // basic block); both K tiles are still in their ring slots.  The second rebase sees the first one's shift.
                if (__any((orv & 0x40004000u) != 0u)) {
                    asm volatile("; rebase");                                   // keeps this rare path a real branch
                    rebase(it, false);
                    rebase(it + 1, false);
                }
                orv = 0;
            }
        }
        for (; it < nt; it += 2) {                    // the last one or two tiles (same ring protocol), masked variant
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (it + 2 < nt) FLASH_ISSUE(it + 2);
            if (it + 3 < nt) FLASH_ISSUE(it + 3);
            tile(it, std::true_type{});
            if (it + 1 < nt) tile(it + 1, std::true_type{});
        }
    } else {
        // ring of NSTG slots, prefetch distance NSTG - 1: tile it+NSTG-1 goes into the slot tile it-1 just left
        FLASH_ISSUE(0);
        if (NSTG == 3 && nt > 1) FLASH_ISSUE(1);
        // (two loops over the same ring protocol -- full tiles, then the at most one tile with padded keys -- so that the hot loop holds
        // only the unmasked body: with both bodies in one loop hipcc's hoisted addressing spilled the d >= 80 kernels)
#define FLASH_STEP(MK)                                                                                                        \
        {                                                                                                                     \
            if (NSTG == 3 && it + 1 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPW) : "memory");                          \
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                             \
            __builtin_amdgcn_s_barrier();             /* every wave's pieces of tile it landed; everyone is done with it-1 */ \
            if (it + NSTG - 1 < nt) FLASH_ISSUE(it + NSTG - 1);                                                               \
            if (SPEC && !decltype(MK)::value && it == 0) rebase(0, true);                                                     \
            tile(it, MK);                                                                                                     \
        }
        int it = 0;
        for (; it < nfull; ++it) FLASH_STEP(std::false_type{})
        for (; it < nt; ++it) FLASH_STEP(std::true_type{})
#undef FLASH_STEP
    }
#undef FLASH_ISSUE
    if constexpr (SPEC) {
        // row sums (O^T row 40) that are not finite and positive: some P left the f16 range -> this block is redone by the gated exact kernel
        bool bad = false;
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            if constexpr (PV16) {
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) { const float l = __shfl(o16[qb][qt][2][0], 32 + (lane & 15), 64); bad |= !(l > 0.f && l < 3e38f); }
            } else { const float l = o[qb][D / 32][4 * ((D % 32) / 8)]; bad |= hl == 0 && !(l > 0.f && l < 3e38f); }     // O^T row D, lanes hl == 0
        }
        const int anybad = __syncthreads_or(bad);
        if (tid == 0) flags[bid] = anybad;
    }
    // ---- epilogue
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        if constexpr (PV16) {
            // O^T row 40 (the ones row: softmax row sums) = tile 2, lanes 32-47, register 0; lane l holds rows 16 t + 4 (l >> 4) + r of query
            // (l & 15) + 16 qt: four consecutive output channels -> one 8-byte store per (qt, t)
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                const float inv = 1.f / __shfl(o16[qb][qt][2][0], 32 + (lane & 15), 64);
                const int q = q0 + qb * 32 + qt * 16 + (lane & 15);
                if (q < Tq) {
                    _Float16* orow = O + (long)b * obstride + (long)q * ldo + head * d;
#pragma unroll
                    for (int t = 0; t < NT16; ++t) {
                        const int dd = t * 16 + 4 * (lane >> 4);
                        if (dd < d) {
                            const float4v v = o16[qb][qt][t];
                            half4 w = {(_Float16)(v[0] * inv), (_Float16)(v[1] * inv), (_Float16)(v[2] * inv), (_Float16)(v[3] * inv)};
                            *(half4*)(orow + dd) = w;
                        }
                    }
                }
            }
            continue;
        }
        float l;
        if (LROW) {      // l sits in O^T row D: tile D/32, register group (D%32)/8 (D%8 == 0), lanes with hl == (D%8)/4 == 0
            constexpr int TL = D / 32, RG = (D % 32) / 8;
            l = o[qb][TL][4 * RG];
            l = __shfl(l, ql, 64);                    // broadcast from the hl == 0 half
        } else {
            l = lsum[qb] + __shfl_xor(lsum[qb], 32, 64);
        }
        const float inv = 1.f / l;
        const int q = q0 + qb * 32 + ql;
        if constexpr (SPLIT) {      // split-KV (k_flash_lse): this entry saw one chunk of the keys -- hand on log2 of its softmax denominator at the shift it used
            if (q < Tq && hl == 0) lse[bh * Tq + q] = m[qb] + __log2f(l);
        }
        if (q < Tq) {
            _Float16* orow = O + (long)b * obstride + (long)q * ldo + head * d;
#pragma unroll
            for (int t = 0; t < NDT; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    int dd = t * 32 + 8 * g + 4 * hl;
                    if (dd < d) {
                        half4 w = {(_Float16)(o[qb][t][4 * g] * inv), (_Float16)(o[qb][t][4 * g + 1] * inv), (_Float16)(o[qb][t][4 * g + 2] * inv), (_Float16)(o[qb][t][4 * g + 3] * inv)};
                        *(half4*)(orow + dd) = w;
                    }
                }
        }
    }
}

template <int D, int DP, int DPV, int QB, int NSTG, int TPB, int MINB, int SPEC>
__global__ __launch_bounds__(256, MINB ? MINB : (QB == 1 && DP <= 80 && TPB == 1 ? 3 : 2)) void k_flash(const _Float16* __restrict__ Qp, const _Float16* __restrict__ Kp, const _Float16* __restrict__ Vt,
                                                  _Float16* __restrict__ O, int H, int Tq, int Tk, int Tqp, int Tkp, int d, int ldo, long obstride,
                                                  int kv_div, int nqb, int* __restrict__ flags, int nblk) {
    if constexpr (D == 40 && QB == 2 && !SPEC) {
        // The exact kernel as the second pass behind the speculative one: normally NO block is flagged, and dispatching B H nqb (~3 000) blocks of
        // 222 VGPRs / 66 KiB LDS just to read one word each took 57 us per attention call on the main stream (1.6 s per 300-frame pass).  The
        // gated pass is launched with at most 512 blocks (one resident round); a block walks the flags of its stride class and runs the flagged ones.
        if (flags) {
            // Round 5, second pass: a block reads its flags 256 at a time (one load per thread, one round trip per window) instead of one after the other
            // -- a block of a 16-block grid walked ~370 DEPENDENT L2 round trips, which is why small grids measured slower (profiles/r5_ab_flash_gate.txt);
            // with the windowed scan a 32-block grid costs the same as 512 IN THE PASS too (profiles/r5c_ab_gate_inpass.txt: 33.12-33.14 s of denoise at
            // 60 frames either way, 8 blocks +0.3 %): the ~52 us of this launch are not a wait for slots between the matching chain's blocks.  512 stays.
            const int per = (nblk + (int)gridDim.x - 1) / (int)gridDim.x, lo = (int)blockIdx.x * per, hi = min(lo + per, nblk);
            for (int base = lo; base < hi; base += 256) {
                const int mine = base + (int)threadIdx.x < hi ? flags[base + threadIdx.x] : 0;
                if (!__syncthreads_or(mine)) continue;
                for (int bid = base; bid < min(base + 256, hi); ++bid) {          // (rare: some block of this window flagged an overflow)
                    if (!flags[bid]) continue;
                    flash_block<D, DP, DPV, QB, NSTG, TPB, MINB, SPEC>(bid, Qp, Kp, Vt, O, H, Tq, Tk, Tqp, Tkp, d, ldo, obstride, kv_div, nqb, flags);
                    __syncthreads();              // the next item re-uses the LDS ring
                }
            }
            return;
        }
    }
    flash_block<D, DP, DPV, QB, NSTG, TPB, MINB, SPEC>(blockIdx.x, Qp, Kp, Vt, O, H, Tq, Tk, Tqp, Tkp, d, ldo, obstride, kv_div, nqb, flags);
}
// k_flash with a K / V panel index per sample (tcl_attention_kvindex_f16): kv_index[b] in [0, Bkv), checked on the host before the launch.  A kernel of
// its own, so that k_flash above compiles to what it was; the gated pass walks the flags exactly as there.
template <int D, int DP, int DPV, int QB, int NSTG, int TPB, int MINB, int SPEC>
__global__ __launch_bounds__(256, MINB ? MINB : (QB == 1 && DP <= 80 && TPB == 1 ? 3 : 2)) void k_flash_kvi(const _Float16* __restrict__ Qp, const _Float16* __restrict__ Kp, const _Float16* __restrict__ Vt,
                                                  _Float16* __restrict__ O, int H, int Tq, int Tk, int Tqp, int Tkp, int d, int ldo, long obstride,
                                                  const int* __restrict__ kv_index, int nqb, int* __restrict__ flags, int nblk) {
    if constexpr (D == 40 && QB == 2 && !SPEC) {
        if (flags) {
            const int per = (nblk + (int)gridDim.x - 1) / (int)gridDim.x, lo = (int)blockIdx.x * per, hi = min(lo + per, nblk);
            for (int base = lo; base < hi; base += 256) {
                const int mine = base + (int)threadIdx.x < hi ? flags[base + threadIdx.x] : 0;
                if (!__syncthreads_or(mine)) continue;
                for (int bid = base; bid < min(base + 256, hi); ++bid) {
                    if (!flags[bid]) continue;
                    flash_block<D, DP, DPV, QB, NSTG, TPB, MINB, SPEC, false, true>(bid, Qp, Kp, Vt, O, H, Tq, Tk, Tqp, Tkp, d, ldo, obstride, 1, nqb, flags, nullptr, kv_index);
                    __syncthreads();
                }
            }
            return;
        }
    }
    flash_block<D, DP, DPV, QB, NSTG, TPB, MINB, SPEC, false, true>(blockIdx.x, Qp, Kp, Vt, O, H, Tq, Tk, Tqp, Tkp, d, ldo, obstride, 1, nqb, flags, nullptr, kv_index);
}

// ---- optional in-library timing of the flash kernel (bench.py roofline leg): HIP events recorded on the launch stream
#include <vector>
#include <deque>
struct FlashProf { bool on = false; int dfilter = 0; std::deque<hipEvent_t> ev; double flops = 0.0, ms = 0.0; long launches = 0; int big[4] = {0, 0, 0, 0}; double bigfl = 0.0; };
static FlashProf g_prof;
// resolve (elapsed time -> g_prof.ms) and free the oldest event pairs: all of them (blocking) or only those already complete
static void flash_prof_drain(bool all) {
    while (g_prof.ev.size() >= 2) {
        hipEvent_t e0 = g_prof.ev[0], e1 = g_prof.ev[1];
        if (all) (void)hipEventSynchronize(e1);
        else if (hipEventQuery(e1) != hipSuccess) break;
        float t = 0.f;
        (void)hipEventElapsedTime(&t, e0, e1);
        g_prof.ms += t;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        g_prof.ev.pop_front(); g_prof.ev.pop_front();
    }
}

// ---- host path: every C-ABI entry fills one AttnCall (check), then pack, choose, run
// One attention call as every host function sees it: the operands (q/k/v/o point at head 0 of batch 0; row strides ld* and batch strides *bs in halves),
// the problem, the decoded TCL_ATTN_* flags, the panel layout with the panels resolved inside ws_q / ws_kv, and the stream.
struct AttnCall {
    const _Float16 *q, *k, *v; int ldq, ldk, ldv; long qbs, kbs, vbs;
    _Float16* o; int ldo; long obs;
    int B, H, Tq, Tk, d; float scale; int kv_div;      // K/V batch index = b / kv_div (kv_div = F for the text cross-attention whose context repeats per frame, else 1)
    bool pack_q, pack_kv, pair;                        // pack_kv = false reuses the K/V panels already in ws_kv (same Bkv, H, Tk, d as the call that packed them)
    AttnPanels p;
    _Float16 *Qp, *Kp, *Vt; int* flags;
    hipStream_t st;
    int Bkv;                                           // entries of the K / V panels: B / kv_div, or kv_rows under a per-sample index
    const int* kv_index;                               // device int32 [B] (NULL: b / kv_div): the K / V entry of every sample, each in [0, Bkv)
};
static bool attn_shape_ok(int B, int H, int Tq, int Tk, int d, int kv_div) {
    return B > 0 && H > 0 && Tq > 0 && Tk > 0 && kv_div > 0 && B % kv_div == 0 && (d == 40 || d == 80 || d == 128 || d == 160);
}
// (shape already checked: kv_div > 0)
static AttnCall attn_call(const void* q, int ldq, long qbs, const void* k, int ldk, long kbs, const void* v, int ldv, long vbs, void* o, int ldo, long obs,
                          int B, int H, int Tq, int Tk, int d, float scale, int kv_div, int flags, void* ws_q, void* ws_kv, hipStream_t st,
                          const int* kv_index = nullptr, int kv_rows = 0) {
    const int Bkv = kv_index ? kv_rows : B / kv_div;
    AttnCall c = {(const _Float16*)q, (const _Float16*)k, (const _Float16*)v, ldq, ldk, ldv, qbs, kbs, vbs, (_Float16*)o, ldo, obs, B, H, Tq, Tk, d, scale, kv_div,
                  !(flags & TCL_ATTN_PREPACKED), (flags & TCL_ATTN_PACK_KV) != 0, (flags & TCL_ATTN_PAIR) != 0, attn_panels(B, Bkv, H, Tq, Tk, d)};
    c.Qp = (_Float16*)ws_q; c.flags = (int*)((char*)ws_q + c.p.flags_off); c.Kp = (_Float16*)ws_kv; c.Vt = c.Kp + c.p.vt_off; c.st = st; c.Bkv = Bkv; c.kv_index = kv_index;
    return c;
}
constexpr size_t flash_lds(int DP, int DPV, int NSTG) {      // NSTG ring slots of one K + V^T image in whole 1-KiB DMA pieces, + the 1-KiB dump
    return (size_t)NSTG * ((KV_TILE * (DP + 8) * 2 + vt_tile_halves(DPV) * 2 + 1023) / 1024) * 1024 + 1024;
}

// One row per flash variant, and what choose() decides for a call: the variant, its launch, and the gated exact pass behind the speculative one
struct FlashVariant { int id; const char* name; int d, qb; size_t lds; int (*run)(const AttnCall&, int grid, bool gated); };
struct FlashPlan { const FlashVariant *v, *second; int grid, grid2; };

template <int D, int QB, int NSTG, int TPB = 1, int MINB = 0, int SPEC = 0>
static int launch_flash(const AttnCall& c, int grid, bool gated) {      // gated: the exact pass behind the speculative launch, over the flagged blocks
    constexpr int DP = attn_dp(D), DPV = attn_dpv(D);
    constexpr size_t lds = flash_lds(DP, DPV, NSTG);
    static bool set = false;
    if (!set) { (void)hipFuncSetAttribute((const void*)k_flash<D, DP, DPV, QB, NSTG, TPB, MINB, SPEC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); set = true; }
    const int nqb = c.p.Tqp / (128 * QB);
    const bool prof = g_prof.on && (g_prof.dfilter == 0 || g_prof.dfilter == c.d);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (prof) {
        if (g_prof.ev.size() > 8192) flash_prof_drain(false);       // a 300-frame pass has ~1e5 launches: keep the live event count bounded
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); (void)hipEventRecord(e0, c.st);
    }
    if (c.kv_index) {
        if constexpr (D != 128) {      // (the text cross-attention's head dims; attention_kvindex refuses 128)
            static bool set_kvi = false;
            if (!set_kvi) { (void)hipFuncSetAttribute((const void*)k_flash_kvi<D, DP, DPV, QB, NSTG, TPB, MINB, SPEC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); set_kvi = true; }
            hipLaunchKernelGGL((k_flash_kvi<D, DP, DPV, QB, NSTG, TPB, MINB, SPEC>), dim3(grid), dim3(256), lds, c.st, c.Qp, c.Kp, c.Vt, c.o, c.H, c.Tq, c.Tk,
                               c.p.Tqp, c.p.Tkp, c.d, c.ldo, c.obs, c.kv_index, nqb, SPEC || gated ? c.flags : nullptr, c.B * c.H * nqb);
        } else return TCL_EINVAL;
    } else {
        hipLaunchKernelGGL((k_flash<D, DP, DPV, QB, NSTG, TPB, MINB, SPEC>), dim3(grid), dim3(256), lds, c.st, c.Qp, c.Kp, c.Vt, c.o, c.H, c.Tq, c.Tk,
                           c.p.Tqp, c.p.Tkp, c.d, c.ldo, c.obs, c.kv_div, nqb, SPEC || gated ? c.flags : nullptr, c.B * c.H * nqb);
    }
    // (the statistics count a call once: the gated pass is timed with the speculative launch it follows)
    if (prof) { (void)hipEventRecord(e1, c.st); g_prof.ev.push_back(e0); g_prof.ev.push_back(e1); if (!gated) { const double fl = 4.0 * c.B * c.H * (double)c.Tq * c.Tk * c.d; g_prof.flops += fl; g_prof.launches++; if (fl > g_prof.bigfl) { g_prof.bigfl = fl; g_prof.big[0] = c.B; g_prof.big[1] = c.H; g_prof.big[2] = c.Tq; g_prof.big[3] = c.Tk; } } }
    return hipPeekAtLastError() == hipSuccess ? TCL_OK : TCL_ELAUNCH;
}
template <int D, int QB, int NSTG, int TPB = 1, int MINB = 0, int SPEC = 0>
constexpr FlashVariant flash_variant(int id, const char* name) {
    return {id, name, D, QB, flash_lds(attn_dp(D), attn_dpv(D), NSTG), launch_flash<D, QB, NSTG, TPB, MINB, SPEC>};
}
// <head_dim, query blocks per wave, ring slots, tiles per barrier, blocks per CU (0: by shape), speculative>; the index is the id tcl_attention_plan reports
enum { FV_40_SPEC, FV_40_QB2, FV_40_QB1, FV_80, FV_128, FV_160, FV_COUNT };
static const FlashVariant g_flash[FV_COUNT] = {
    // d = 40: two query blocks per wave (shared K/V fragments), 4-slot ring and two tiles per barrier, 2 blocks per CU (750 TFLOP/s at T = 35.6k).
    // Speculative softmax (no row maxima in the loop), then the exact kernel over the blocks that flagged an f16 overflow of P (normally none)
    flash_variant<40, 2, 4, 2, 0, 1>(FV_40_SPEC, "d40 qb2 speculative"),
    flash_variant<40, 2, 4, 2>(FV_40_QB2, "d40 qb2 exact"),
    // one query block per wave on a 2-slot ring at 4 blocks per CU (107 VGPRs: four waves per SIMD hide each other's softmax; 582 TFLOP/s at T = 8.9k)
    flash_variant<40, 1, 2, 1, 4>(FV_40_QB1, "d40 qb1"),
    // d = 80: one block, 2-slot ring (50 KB LDS -> 3 blocks per CU).  The kernel moves 24.5 KiB of K / V^T image per 128 queries and tile through
    // LDS-DMA -- ~40 B / clk / CU at three blocks per CU, the measured ceiling of that path (profiles/r3_lds_dma_rate.txt)
    flash_variant<80, 1, 2>(FV_80, "d80"),
    // d = 128, MemFlowNet memory read: ONE head, ONE entry -- at 1280x720 14 400 queries are 114 blocks of 128 for 256 CUs (507 us per call, 0.17 of peak,
    // profiles/r6_memflow_kernel_stats_before.txt).  2-wave blocks (twice the blocks) made the frame pair SLOWER, 47.7 against 45.9 ms
    // (profiles/r6_ab_memflow_graph_nw.txt): the kernel is not simply grid-limited (tcl_attention_splitkv_f16 below cuts the keys instead)
    flash_variant<128, 1, 2>(FV_128, "d128"),
    flash_variant<160, 1, 3>(FV_160, "d160"),
};
// TCL_FLASH40: 0 = choose() as it stands (default), 1 = always the one-query-block kernel, 5 = no speculative softmax (the exact two-query-block
// kernel alone: the kill switch; tools/micro/prec_attn.py, bench_attn_long.py).  Any other value behaves as 0.  Read once per process.
static int flash40_mode() { static const int m = [] { const char* e = getenv("TCL_FLASH40"); const int v = e ? atoi(e) : 0; return v == 1 || v == 5 ? v : 0; }(); return m; }
// Which variant a call gets, with its grid and LDS bytes.  No HIP call: tcl_attention_plan asks it without a GPU.
static FlashPlan choose(const AttnCall& c, int flash40) {
    // d = 40 takes the two-query-block kernels when the grid still fills the chip several times over (pair: counted as for the 2 B samples of the pair)
    const bool qb2 = (long)c.B * (c.pair ? 2 : 1) * c.H * (c.p.Tqp / 256) >= 1024;
    const int id = c.d == 40 ? (qb2 && flash40 != 1 ? (flash40 == 0 ? FV_40_SPEC : FV_40_QB2) : FV_40_QB1) : c.d == 80 ? FV_80 : c.d == 128 ? FV_128 : FV_160;
    const FlashVariant& v = g_flash[id];
    FlashPlan pl = {&v, nullptr, c.B * c.H * (c.p.Tqp / (128 * v.qb)), 0};
    // gated exact pass: a small grid of blocks walks the flags (normally none is set: what the launch costs is the DISPATCH of its 222-VGPR / 66-KiB blocks --
    // 57 us with one block per flag (round 3), 56 us in the pass with one resident round of 512 (round 4).  Round 5 measured smaller grids
    // (profiles/r5_ab_flash_gate.txt): 64 blocks the same call rate as 512, 16 blocks 1.4 % SLOWER -- the pass is not dispatch-bound)
    constexpr int GATE_BLOCKS = 512;
    if (id == FV_40_SPEC) { pl.second = &g_flash[FV_40_QB2]; pl.grid2 = pl.grid > GATE_BLOCKS ? GATE_BLOCKS : pl.grid; }
    return pl;
}

// ---- round 6: split-KV for the MemFlowNet memory read (head_dim 128, ONE head, ONE entry: 14 400 queries are 114 blocks for 256 CUs -- 512 us per call,
// 0.17 of peak, a quarter of a frame pair).  The keys are cut into `nsplit` chunks that ride as batch entries (the Q panel is packed once per chunk, the
// K / V^T panels of a chunk are a batch entry's), every entry writes its normalised partial output and log2 of its denominator, and k_attn_merge joins them:
// O = sum_s 2^(lse_s - max) O_s / sum_s 2^(lse_s - max).  Same kernel body as k_flash<128, ...> (flash_block with SPLIT).
template <int D, int DP, int DPV, int QB, int NSTG>
__global__ __launch_bounds__(256, 2) void k_flash_lse(const _Float16* __restrict__ Qp, const _Float16* __restrict__ Kp, const _Float16* __restrict__ Vt,
                                                      _Float16* __restrict__ O, int H, int Tq, int Tk, int Tqp, int Tkp, int d, int ldo, long obstride, int nqb,
                                                      float* __restrict__ lse) {
    flash_block<D, DP, DPV, QB, NSTG, 1, 0, 0, true>(blockIdx.x, Qp, Kp, Vt, O, H, Tq, Tk, Tqp, Tkp, d, ldo, obstride, 1, nqb, nullptr, lse);
}
// parts [S][Tq][HD] f16, lse [S][H][Tq] -> out [Tq][ldo] (first HD columns)
__global__ void k_attn_merge(const _Float16* __restrict__ parts, const float* __restrict__ lse, _Float16* __restrict__ out, int S, int H, int Tq, int d, int ldo) {
    const int HD = H * d, nchunk = HD / 8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)Tq * nchunk; i += (long)gridDim.x * blockDim.x) {
        const int q = (int)(i / nchunk), c8 = (int)(i % nchunk) * 8, h = c8 / d;
        float mx = -3.0e38f;
        for (int sidx = 0; sidx < S; ++sidx) mx = fmaxf(mx, lse[((long)sidx * H + h) * Tq + q]);
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, wsum = 0.f;
        for (int sidx = 0; sidx < S; ++sidx) {
            const float wgt = exp2f(lse[((long)sidx * H + h) * Tq + q] - mx);
            const half8 pv = *(const half8*)(parts + ((long)sidx * Tq + q) * HD + c8);
            wsum += wgt;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += wgt * (float)pv[j];
        }
        const float inv = 1.f / wsum;
        half8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (_Float16)(acc[j] * inv);
        *(half8*)(out + (long)q * ldo + c8) = o;
    }
}
// the workspace of a split-KV call: [Q panels | K / V^T panels | parts | lse], each part 1-KiB aligned; the panels are those of nsplit entries of one chunk
struct SplitKvWs { AttnPanels p; size_t kv_off, parts_off, lse_off, bytes; };
static SplitKvWs splitkv_ws(int nsplit, int H, int Tq, int Tk, int d) {
    SplitKvWs w = {attn_panels(nsplit, nsplit, H, Tq, Tk / (nsplit > 0 ? nsplit : 1), d)};
    w.kv_off = attn_rup(w.p.q_bytes, 1024); w.parts_off = w.kv_off + attn_rup(w.p.kv_bytes, 1024);
    w.lse_off = w.parts_off + attn_rup((size_t)nsplit * Tq * H * d * 2, 1024); w.bytes = w.lse_off + (size_t)nsplit * H * Tq * 4 + 1024;
    return w;
}

// The Q (scaled), K and V^T panels of a call, as its pack_q / pack_kv ask: one launch when both are packed.
static int attention_pack(const AttnCall& c) {
    const AttnPanels& p = c.p;
    const int Bkv = c.Bkv, nt = p.Tkp / KV_TILE;
    const long qc = (long)c.B * c.H * p.Tqp * (p.DP / 8), kc = (long)Bkv * c.H * p.Tkp * (p.KS / 8);
    const int gq = stream_grid(qc, 256, 2), gk = stream_grid(kc, 256, 2);
    const size_t vt_lds = (size_t)64 * (p.DPV + 2) * 2;
    const PackRows pq = {c.q, c.qbs, c.ldq, c.Tq, c.d, AttnPanels::qscale(c.scale), c.Qp, p.Tqp, p.DP, qc, -1};
    const PackRows pk = {c.k, c.kbs, c.ldk, c.Tk, c.d, 1.f, c.Kp, p.Tkp, p.KS, kc, p.one_col};
    auto rows = [&](const PackRows& r, int grid) {
        hipLaunchKernelGGL(k_pack_rows, dim3(grid), dim3(256), 0, c.st, r.src, r.bstride, r.ld, r.T, c.H, r.d, r.scale, r.dst, r.Tp, r.DP, r.total, r.one_col);
    };
    if (c.pack_q && c.pack_kv)
        hipLaunchKernelGGL(k_pack_qkv, dim3(gq + gk + nt * Bkv * c.H), dim3(256), vt_lds, c.st, pq, pk, gq, gk, c.H, c.v, c.vbs, c.ldv, c.Tk, c.d, c.Vt, nt, p.DPV, p.skew);
    else {
        if (c.pack_q) rows(pq, gq);
        if (c.pack_kv) rows(pk, gk);
        if (c.pack_kv) hipLaunchKernelGGL(k_pack_vt, dim3(nt, Bkv * c.H), dim3(256), vt_lds, c.st, c.v, c.vbs, c.ldv, c.Tk, c.H, c.d, c.Vt, nt, p.DPV, p.skew);
    }
    return hipPeekAtLastError() == hipSuccess ? TCL_OK : TCL_ELAUNCH;
}

// pack (as the call's flags ask), choose, run
static int attention_run(const AttnCall& c) {
    if (attention_pack(c) != TCL_OK) return TCL_ELAUNCH;
    const FlashPlan pl = choose(c, flash40_mode());
    int rc = pl.v->run(c, pl.grid, false);
    if (rc == TCL_OK && pl.second) rc = pl.second->run(c, pl.grid2, true);
    return rc;
}

extern "C" {

// Timing of the flash kernel launches (all head dims, or only head_dim == dfilter) with HIP events on their stream.
int tcl_flash_profile_begin(int dfilter) { g_prof.on = true; g_prof.dfilter = dfilter; g_prof.flops = 0.0; g_prof.ms = 0.0; g_prof.launches = 0; g_prof.bigfl = 0.0; g_prof.ev.clear(); return TCL_OK; }
// -> (B, H, Tq, Tk) of the largest launch profiled since begin
int tcl_flash_profile_shape(int* shape4) { TCL_CHECK_ARG(shape4); for (int i = 0; i < 4; ++i) shape4[i] = g_prof.big[i]; return TCL_OK; }
// -> total kernel ms, algorithmic FLOPs (4*B*H*Tq*Tk*d per launch) and launch count since begin; synchronises the events.
int tcl_flash_profile_end(double* total_ms, double* total_flops, long* launches) {
    TCL_CHECK_ARG(total_ms && total_flops && launches);
    flash_prof_drain(true);
    const double ms = g_prof.ms;
    *total_ms = ms; *total_flops = g_prof.flops; *launches = g_prof.launches;
    g_prof.on = false; g_prof.ev.clear();
    return TCL_OK;
}

// panel sizes (AttnPanels): the Q panel + per-block flags; the K and V^T panels
size_t tcl_attention_q_bytes(int B, int H, int Tq, int d) { return attn_panels(B, 0, H, Tq, 0, d).q_bytes; }
size_t tcl_attention_kv_bytes(int Bkv, int H, int Tk, int d) { return attn_panels(0, Bkv, H, 0, Tk, d).kv_bytes; }

// The packing half of tcl_attention_f16 on its own (same panels, same workspace layout): Q (scaled) and, with TCL_ATTN_PACK_KV, K / V^T.  A caller that
// runs it on another stream than the attention itself passes TCL_ATTN_PREPACKED (and no TCL_ATTN_PACK_KV) to tcl_attention_f16 afterwards.
int tcl_attention_pack_f16(const void* q, int ldq, long qbs, const void* k, int ldk, long kbs, const void* v, int ldv, long vbs, int B, int H, int Tq,
                           int Tk, int d, float scale, int kv_div, int pack_kv, void* ws_q, void* ws_kv, hipStream_t st) {
    TCL_CHECK_ARG(q && ws_q && ws_kv && attn_shape_ok(B, H, Tq, Tk, d, kv_div));
    TCL_CHECK_ARG(!(pack_kv & TCL_ATTN_PACK_KV) || (k && v));
    return attention_pack(attn_call(q, ldq, qbs, k, ldk, kbs, v, ldv, vbs, nullptr, 0, 0, B, H, Tq, Tk, d, scale, kv_div, pack_kv & TCL_ATTN_PACK_KV, ws_q, ws_kv, st));
}
// attn1's QKV projection of ne x T merged tokens (x [ne*T, K] @ W[3 H d, K]^T, no bias: diffusers Attention.to_q / to_k / to_v) written straight into
// the panels tcl_attention_pack_f16 would have produced from its [ne*T, 3 H d] output -- same bits in every byte the pack writes.
// x: entry b's rows start at x + b * x_bs (elements); row_index (may be NULL): merged token t = row row_index[t] of the entry's block -- the VidToMe merge
// map applied in the GEMM's operand load (merge.py "replace" mode is a pure gather), so the merged sequence needs no tensor of its own.  ws_q / ws_kv must have
// been ZERO-INITIALISED once for this (ne, H, T, d) (sizes: tcl_attention_q_bytes / _kv_bytes) and may be reused by stream-ordered calls of the same shape:
// padding rows / columns and the V^T rows above the ones row are never written.  Follow with tcl_attention_f16(..., TCL_ATTN_PREPACKED | pair bit, ws_q, ws_kv).
int tcl_gemm_qkv_panels_f16(const void* x, long x_bs, const int* row_index, const void* W, int ne, int T, int H, int d, int K, int ldx, int ldw, float scale,
                            void* ws_q, void* ws_kv, hipStream_t st) {
    TCL_CHECK_ARG(x && W && ws_q && ws_kv && ne > 0 && T > 0 && H > 0 && (d == 40 || d == 80) && K > 0 && K % 32 == 0 && ldx >= K && ldw >= K);
    const AttnPanels p = attn_panels(ne, ne, H, T, T, d);
    const QkvPanel qp = {(_Float16*)ws_q, (_Float16*)ws_kv, (_Float16*)ws_kv + p.vt_off, T, p.Tqp, p.Tkp, H, d, p.DP, p.KS, p.DPV, p.vtile, p.one_col, p.skew,
                         AttnPanels::qscale(scale), row_index, x_bs};
    TclProfScope ps(TCL_PROF_GEMM, st, 2.0 * ne * T * 3.0 * H * d * K);
    return gemm_dma_qkv_panels((const _Float16*)x, (const _Float16*)W, ne, K, ldx, ldw, qp, st);
}
// softmax(Q K^T * scale) V per head: check, pack, choose, run.
int tcl_attention_f16(const void* q, int ldq, long qbs, const void* k, int ldk, long kbs, const void* v, int ldv, long vbs, void* o, int ldo,
                      long obs, int B, int H, int Tq, int Tk, int d, float scale, int kv_div, int pack_kv, void* ws_q, void* ws_kv,
                      hipStream_t st) {
    TCL_CHECK_ARG(q && o && ws_q && ws_kv && attn_shape_ok(B, H, Tq, Tk, d, kv_div));
    TCL_CHECK_ARG(!(pack_kv & TCL_ATTN_PACK_KV) || ((k && v) && !(pack_kv & TCL_ATTN_PREPACKED)));
    return attention_run(attn_call(q, ldq, qbs, k, ldk, kbs, v, ldv, vbs, o, ldo, obs, B, H, Tq, Tk, d, scale, kv_div, pack_kv, ws_q, ws_kv, st));
}
// tcl_attention_f16 with the K / V entry of every sample read from a table (generation.prompt_path: every frame its own text).  kv_index NULL: that call.
int tcl_attention_kvindex_f16(const void* q, int ldq, long qbs, const void* k, int ldk, long kbs, const void* v, int ldv, long vbs, void* o, int ldo,
                              long obs, int B, int H, int Tq, int Tk, int d, float scale, int kv_div, int pack_kv, void* ws_q, void* ws_kv,
                              const int* kv_index, const int* h_kv_index, int kv_rows, hipStream_t st) {
    if (!kv_index) return tcl_attention_f16(q, ldq, qbs, k, ldk, kbs, v, ldv, vbs, o, ldo, obs, B, H, Tq, Tk, d, scale, kv_div, pack_kv, ws_q, ws_kv, st);
    TCL_CHECK_ARG(q && o && ws_q && ws_kv && attn_shape_ok(B, H, Tq, Tk, d, 1) && d != 128 && h_kv_index && kv_rows > 0);
    TCL_CHECK_ARG(!(pack_kv & TCL_ATTN_PACK_KV) || ((k && v) && !(pack_kv & TCL_ATTN_PREPACKED)));
    for (int b = 0; b < B; ++b) TCL_CHECK_ARG(h_kv_index[b] >= 0 && h_kv_index[b] < kv_rows);      // the host copy of the table: nothing is launched on a bad one
    return attention_run(attn_call(q, ldq, qbs, k, ldk, kbs, v, ldv, vbs, o, ldo, obs, B, H, Tq, Tk, d, scale, 1, pack_kv, ws_q, ws_kv, st, kv_index, kv_rows));
}
// What choose() decides for tcl_attention_f16(..., flags, ...): out4 = (variant id, blocks of its launch, blocks of the gated exact launch behind the
// speculative kernel or 0, dynamic LDS bytes).  Pure host code.
int tcl_attention_plan(int B, int H, int Tq, int Tk, int d, int kv_div, int flags, int* out4) {
    TCL_CHECK_ARG(out4 && attn_shape_ok(B, H, Tq, Tk, d, kv_div) && !((flags & TCL_ATTN_PACK_KV) && (flags & TCL_ATTN_PREPACKED)));
    const FlashPlan pl = choose(attn_call(nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0, B, H, Tq, Tk, d, 1.f, kv_div, flags, nullptr, nullptr, nullptr), flash40_mode());
    out4[0] = pl.v->id; out4[1] = pl.grid; out4[2] = pl.grid2; out4[3] = (int)pl.v->lds;
    return TCL_OK;
}

// Split-KV attention for one entry (B = 1): see k_flash_lse.  q [Tq, ldq], k [Tk, ldk], v [Tk, ldv] (head h at column h d), o [Tq, ldo].
// Tk must be a multiple of 64 nsplit; d = 128.  ws: tcl_attention_splitkv_workspace_bytes(nsplit, H, Tq, Tk, d).
size_t tcl_attention_splitkv_workspace_bytes(int nsplit, int H, int Tq, int Tk, int d) { return splitkv_ws(nsplit, H, Tq, Tk, d).bytes; }
int tcl_attention_splitkv_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int H, int Tq, int Tk, int d,
                              float scale, int nsplit, void* ws, hipStream_t st) {
    TCL_CHECK_ARG(q && k && v && o && ws && H > 0 && Tq > 0 && Tk > 0 && d == 128 && nsplit >= 2 && nsplit <= 16 && Tk % (64 * nsplit) == 0 && ldo >= H * d);
    const SplitKvWs w = splitkv_ws(nsplit, H, Tq, Tk, d);
    const int chunk = Tk / nsplit;
    char* base = (char*)ws;
    _Float16* parts = (_Float16*)(base + w.parts_off); float* lse = (float*)(base + w.lse_off);
    // the per-chunk view: nsplit batch entries share the queries (batch stride 0) and own one chunk of the keys each; entry s writes parts[s]
    const AttnCall c = attn_call(q, ldq, 0, k, ldk, (long)chunk * ldk, v, ldv, (long)chunk * ldv, parts, H * d, (long)Tq * H * d, nsplit, H, Tq, chunk, d, scale, 1,
                                 TCL_ATTN_PACK_KV, base, base + w.kv_off, st);
    if (attention_pack(c) != TCL_OK) return TCL_ELAUNCH;
    constexpr size_t lds = flash_lds(128, 128, 2);
    static bool set = false;
    if (!set) { (void)hipFuncSetAttribute((const void*)k_flash_lse<128, 128, 128, 1, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); set = true; }
    const int nqb = c.p.Tqp / 128;
    hipLaunchKernelGGL((k_flash_lse<128, 128, 128, 1, 2>), dim3(nsplit * H * nqb), dim3(256), lds, st, c.Qp, c.Kp, c.Vt, c.o, H, Tq, chunk, c.p.Tqp, c.p.Tkp, d, c.ldo,
                       c.obs, nqb, lse);
    hipLaunchKernelGGL(k_attn_merge, dim3(stream_grid((long)Tq * (H * d / 8), 256, 2)), dim3(256), 0, st, parts, lse, (_Float16*)o, nsplit, H, Tq, d, ldo);
    TCL_LAUNCH_RET();
}

}  // extern "C"
