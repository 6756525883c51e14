// generation.prompt_path: the text conditioning of a frame between two keyframe prompts -- a linear blend of the two keyframes' CLIP
// last_hidden_state [L, D] f16, one launch for all frames (include/tclight_hip.h: tcl_text_lerp_f16 states the float sequence).
#include "common.h"
#include "../../include/tclight_hip.h"
#include <string.h>

typedef _Float16 lerp_h8 __attribute__((ext_vector_type(8)));

// tab [F][3] int32 = (k0, k1, bits of t as f32): a block serves one frame (blockIdx.y), so the three are scalar loads.  t == 0 / t == 1 copy the bits
// of keyframe k0 / k1 (a + 0 (b - a) would turn -0 into +0, a + 1 (b - a) need not be b); otherwise, every operation rounded to f32 on its own,
// a32 = f32(a); b32 = f32(b); e = b32 - a32; m = t * e; s = a32 + m; out = f16(s).
// VEC: LD % 8 == 0 and both bases 16 B aligned -> a lane owns 8 consecutive elements: two 16 B loads, one 16 B store.
template <bool VEC>
__global__ __launch_bounds__(256) void k_text_lerp(_Float16* __restrict__ out, const _Float16* __restrict__ keys, const int* __restrict__ tab, long LD) {
#pragma clang fp contract(off)
    constexpr int V = VEC ? 8 : 1;
    const int f = blockIdx.y;
    const int k0 = tab[3 * f], k1 = tab[3 * f + 1];
    const float t = __int_as_float(tab[3 * f + 2]);
    const _Float16* pa = keys + (long)k0 * LD;
    const _Float16* pb = keys + (long)k1 * LD;
    _Float16* po = out + (long)f * LD;
    const long per = LD / V;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < per; g += (long)gridDim.x * blockDim.x) {
        const long i = g * V;
        if (t == 0.f || t == 1.f) {                       // (uniform over the block)
            const _Float16* src = (t == 0.f ? pa : pb) + i;
            if (VEC) *(lerp_h8*)(po + i) = *(const lerp_h8*)src; else po[i] = *src;
        } else if (VEC) {
            const lerp_h8 a = *(const lerp_h8*)(pa + i), b = *(const lerp_h8*)(pb + i);
            lerp_h8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float a32 = (float)a[j], e = (float)b[j] - a32;
                const float m = t * e;
                const float s = a32 + m;
                o[j] = (_Float16)s;
            }
            *(lerp_h8*)(po + i) = o;
        } else {
            const float a32 = (float)pa[i], e = (float)pb[i] - a32;
            const float m = t * e;
            const float s = a32 + m;
            po[i] = (_Float16)s;
        }
    }
}

extern "C" {

int tcl_text_lerp_f16(void* out, const void* keys, int n_keys, const int* tab, const int* h_tab, int F, long LD, hipStream_t st) {
    TCL_CHECK_ARG(out && keys && tab && h_tab && n_keys > 0 && F > 0 && F <= 65535 && LD > 0);
    for (int f = 0; f < F; ++f) {                          // the host copy of the table: nothing is launched on a bad one
        float t;
        memcpy(&t, &h_tab[3 * f + 2], sizeof t);
        TCL_CHECK_ARG(h_tab[3 * f] >= 0 && h_tab[3 * f] < n_keys && h_tab[3 * f + 1] >= 0 && h_tab[3 * f + 1] < n_keys && t >= 0.f && t <= 1.f);
    }
    const bool vec = LD % 8 == 0 && (((uintptr_t)out | (uintptr_t)keys) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(k_text_lerp<true>, dim3(stream_grid(LD / 8, 256, 1), F), dim3(256), 0, st, (_Float16*)out, (const _Float16*)keys, tab, LD);
    else
        hipLaunchKernelGGL(k_text_lerp<false>, dim3(stream_grid(LD, 256, 1), F), dim3(256), 0, st, (_Float16*)out, (const _Float16*)keys, tab, LD);
    TCL_LAUNCH_RET();
}

}  // extern "C"
