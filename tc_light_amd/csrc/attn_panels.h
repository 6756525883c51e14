// The panel layout of one attention call, defined ONCE: what the pack kernels and the two panel-writing GEMM epilogues (gemm.hip: QKV panels, linstrip.hip:
// Q panel) write, what the flash kernels read and what the *_bytes functions of the C ABI promise.  csrc/attn.hip documents the panels themselves.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#define KV_TILE 64
#define V_STRIDE 72   // halves: 144 B = 9 x 16 B (odd) -> the 16-lane groups of a ds_read_b128 are conflict-free
// V^T tile of 64 keys: DPV rows of V_STRIDE halves.  Head_dim 40 stores 64 rows (9 KiB per tile, 16 DMA pieces per 64-key stage with the 7 KiB K
// image), of which its PV on 16x16x32 MFMAs reads 48 (40 + the ones row + 7 idle).
__host__ __device__ constexpr int vt_tile_halves(int dpv) { return dpv * V_STRIDE; }
// Q / K rows hold DP = ceil16(d) halves (K rows KS = DP + 8: KS / 8 odd -> conflict-free b128 reads), the V^T tile DPV = ceil32(d) rows
__host__ __device__ constexpr int attn_dp(int d) { return (d + 15) / 16 * 16; }
__host__ __device__ constexpr int attn_dpv(int d) { return (d + 31) / 32 * 32; }
constexpr size_t attn_rup(size_t x, size_t m) { return (x + m - 1) / m * m; }
constexpr float TCL_LOG2E = 1.4426950408889634f;

struct AttnPanels {
    int Tqp, Tkp, DP, KS, DPV, vtile;      // ceil256(Tq), ceil64(Tk), see above; halves of one V^T tile
    int one_col;      // head_dim 40: K column d is 1 in valid rows (the folded softmax shift rides in Q column d against it); else -1
    int skew;         // head_dim 40 (PV on 16x16x32 MFMAs) reads the V^T tile with rows 4..11 (mod 16) skewed, see pack_vt_blk
    size_t qpanel_bytes, flags_bytes, flags_off;      // ws_q: Qp [B, H, Tqp, DP], then (256-B aligned) one int per 128-query block
    size_t vt_off;                                    // ws_kv: Kp [Bkv, H, Tkp, KS], then Vt [Bkv, H, Tkp / 64, vtile] vt_off HALVES in (1-KiB aligned)
    size_t q_bytes, kv_bytes;                         // what tcl_attention_q_bytes / _kv_bytes answer
    static float qscale(float softmax_scale) { return softmax_scale * TCL_LOG2E; }      // folded into the Q panel: the kernels exponentiate with exp2
};
// A producer of the Q panel alone passes Bkv = Tk = 0.
inline AttnPanels attn_panels(int B, int Bkv, int H, int Tq, int Tk, int d) {
    AttnPanels p;
    p.Tqp = (int)attn_rup(Tq, 256); p.Tkp = (int)attn_rup(Tk, KV_TILE); p.DP = attn_dp(d); p.KS = p.DP + 8; p.DPV = attn_dpv(d);
    p.vtile = vt_tile_halves(p.DPV); p.one_col = d == 40 ? d : -1; p.skew = d == 40;
    p.qpanel_bytes = (size_t)B * H * p.Tqp * p.DP * 2; p.flags_bytes = (size_t)B * H * (p.Tqp / 128) * 4; p.flags_off = attn_rup(p.qpanel_bytes, 256);
    p.q_bytes = p.qpanel_bytes + 256 + p.flags_bytes;
    const size_t k_halves = (size_t)Bkv * H * p.Tkp * p.KS;
    p.vt_off = attn_rup(k_halves, 512);
    p.kv_bytes = (k_halves + (size_t)Bkv * H * (p.Tkp / KV_TILE) * p.vtile) * 2 + 2048;
    return p;
}
