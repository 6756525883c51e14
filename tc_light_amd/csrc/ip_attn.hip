// generation.ip_adapter: IP-Adapter's decoupled image cross-attention, added into the text cross-attention's output in place --
// a += ip_scale * softmax(q K_ip^T * qk_scale) V_ip over Tip <= 16 image tokens (include/tclight_hip.h: tcl_attention_ip_add_f16 states the float
// sequence).  One pass over q and a: 6 B of HBM per element of [M, C] (q read, a read and written); that stream is the bound to aim at (measured:
// 2.6 TB/s at d = 40, 1.6 - 1.7 TB/s at d = 80 / 160 on an MI355X).
//
// Mapping: one thread per (query row, head).  The 8 heads of a row sit in 8 consecutive lanes, so a wave covers 8 whole rows and a 256-thread block
// 32; every access of q and a is a 16 B load / store (global_load_dwordx4) and, over the d / 8 chunks of a head, each cache line a wave touches is
// used whole.  K_ip | V_ip of the block's batch entry are staged once per block into LDS and the block then walks the row tiles of its sample, so the
// staging is amortised over Tq / gridDim.x rows.  In LDS a head's row of d halves is held at a stride of HS halves with HS / 8 odd (40, 88, 168):
// the lanes of a ds_read_b128 group that hold distinct heads then fall on distinct 16 B slots of the 256 B bank row (lanes of equal head read one
// address, which broadcasts); at the natural strides 80 and 160 the 8 heads would share 4 and 2 slots.
#include "common.h"
#include "../../include/tclight_hip.h"

typedef _Float16 ip_h8 __attribute__((ext_vector_type(8)));

__host__ __device__ constexpr int ip_head_stride(int d) { return d == 40 ? 40 : d + 8; }

// TMAX: the unrolled token count (4 or 16); tokens t >= Tip are skipped by a uniform branch.
template <int D, int TMAX>
__global__ __launch_bounds__(256) void k_ip_add(const _Float16* __restrict__ q, int ldq, long qbs, const _Float16* __restrict__ kv, _Float16* a, int lda,
                                                long abs_, int H, int Tq, int Tip, float qk_scale, float ip_scale, int kv_div) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) _Float16 ip_sm[];
    constexpr int HS = ip_head_stride(D);
    const int b = blockIdx.y, C = H * D;
    _Float16* Ks = ip_sm;
    _Float16* Vs = ip_sm + Tip * H * HS;
    const _Float16* src = kv + (long)(b / kv_div) * Tip * 2 * C;
    const int cpr = C / 8;                                   // 16 B chunks of a K (or V) row; a chunk never straddles two heads (D % 8 == 0)
    for (int i = threadIdx.x; i < Tip * 2 * cpr; i += blockDim.x) {
        const int t = i / (2 * cpr), c = i - t * 2 * cpr;
        const bool isv = c >= cpr;
        const int cc = isv ? c - cpr : c;
        const int h = cc * 8 / D, off = cc * 8 - h * D;
        *(ip_h8*)((isv ? Vs : Ks) + (t * H + h) * HS + off) = *(const ip_h8*)(src + (long)t * 2 * C + (long)c * 8);
    }
    __syncthreads();
    const int rows = blockDim.x / H;
    const int h = threadIdx.x % H, rl = threadIdx.x / H;
    for (int r = blockIdx.x * rows + rl; r < Tq; r += gridDim.x * rows) {
        const _Float16* qp = q + (long)b * qbs + (long)r * ldq + h * D;
        float s[TMAX];
#pragma unroll
        for (int t = 0; t < TMAX; ++t) s[t] = 0.f;
#pragma unroll
        for (int j = 0; j < D / 8; ++j) {
            const ip_h8 qv = *(const ip_h8*)(qp + 8 * j);
#pragma unroll
            for (int t = 0; t < TMAX; ++t) {
                if (t < Tip) {
                    const ip_h8 kk = *(const ip_h8*)(Ks + (t * H + h) * HS + 8 * j);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float p = (float)qv[e] * (float)kk[e];
                        s[t] = s[t] + p;
                    }
                }
            }
        }
        float m = s[0] * qk_scale;
        s[0] = m;
#pragma unroll
        for (int t = 1; t < TMAX; ++t)
            if (t < Tip) {
                s[t] = s[t] * qk_scale;
                m = fmaxf(m, s[t]);
            }
        float l = 0.f;
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
            if (t < Tip) {
                s[t] = expf(s[t] - m);
                l = t == 0 ? s[0] : l + s[t];
            }
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
            if (t < Tip) s[t] = s[t] / l;
        _Float16* ap = a + (long)b * abs_ + (long)r * lda + h * D;
#pragma unroll
        for (int j = 0; j < D / 8; ++j) {
            const ip_h8 av = *(const ip_h8*)(ap + 8 * j);
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
            for (int t = 0; t < TMAX; ++t) {
                if (t < Tip) {
                    const ip_h8 vv = *(const ip_h8*)(Vs + (t * H + h) * HS + 8 * j);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float p = s[t] * (float)vv[e];
                        o[e] = o[e] + p;
                    }
                }
            }
            ip_h8 out;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float term = ip_scale * o[e];
                const float sum = (float)av[e] + term;
                out[e] = term == 0.f ? av[e] : (_Float16)sum;      // a zero term keeps a's bits (-0 + 0 would be +0)
            }
            *(ip_h8*)(ap + 8 * j) = out;
        }
    }
}

template <int D, int TMAX>
static int ip_launch(const void* q, int ldq, long qbs, const void* kv, void* a, int lda, long abs_, int B, int H, int Tq, int Tip, float qk_scale,
                     float ip_scale, int kv_div, hipStream_t st) {
    const size_t lds = (size_t)2 * Tip * H * ip_head_stride(D) * sizeof(_Float16);
    // above 48 KB (Tip = 16 at d = 160: 84 KB) the kernel needs the attribute on the CURRENT device: set on every such call (a host-side
    // setting, no launch), so a second device or thread of the process gets it too
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute((const void*)k_ip_add<D, TMAX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return TCL_ELAUNCH;
    const int rows = 256 / H;
    const int tiles = cdiv(Tq, rows);
    int gx = 8192 / B;                                       // about 256 CUs x 8 blocks x 4 over the samples; the rest is walked by the row loop
    gx = gx < 1 ? 1 : (gx > tiles ? tiles : gx);
    hipLaunchKernelGGL((k_ip_add<D, TMAX>), dim3(gx, B), dim3(256), lds, st, (const _Float16*)q, ldq, qbs, (const _Float16*)kv, (_Float16*)a, lda, abs_,
                       H, Tq, Tip, qk_scale, ip_scale, kv_div);
    TCL_LAUNCH_RET();
}

extern "C" {

int tcl_attention_ip_add_f16(const void* q, int ldq, long qbs, const void* kv_ip, void* a, int lda, long abs_, int B, int H, int Tq, int Tip, int d,
                             float qk_scale, float ip_scale, int kv_div, hipStream_t st) {
    TCL_CHECK_ARG(q && kv_ip && a);
    TCL_CHECK_ARG(Tip >= 1 && Tip <= 16 && (d == 40 || d == 80 || d == 160));
    TCL_CHECK_ARG(B >= 1 && B <= 65535 && kv_div >= 1 && B % kv_div == 0 && Tq >= 1);
    TCL_CHECK_ARG(H >= 1 && H <= 8 && 256 % H == 0);
    TCL_CHECK_ARG(ldq >= H * d && lda >= H * d && ldq % 8 == 0 && lda % 8 == 0 && qbs % 8 == 0 && abs_ % 8 == 0);
    TCL_CHECK_ARG(B == 1 || (qbs >= (long)(Tq - 1) * ldq + H * d && abs_ >= (long)(Tq - 1) * lda + H * d));
    TCL_CHECK_ARG((((uintptr_t)q | (uintptr_t)kv_ip | (uintptr_t)a) & 15) == 0);
    if (ip_scale == 0.f) return TCL_OK;                      // the term is zero: a stays as it is, nothing is launched
#define IP_GO(D) return Tip <= 4 ? ip_launch<D, 4>(q, ldq, qbs, kv_ip, a, lda, abs_, B, H, Tq, Tip, qk_scale, ip_scale, kv_div, st) \
                                 : ip_launch<D, 16>(q, ldq, qbs, kv_ip, a, lda, abs_, B, H, Tq, Tip, qk_scale, ip_scale, kv_div, st)
    if (d == 40) IP_GO(40);
    if (d == 80) IP_GO(80);
    IP_GO(160);
#undef IP_GO
}

}  // extern "C"
