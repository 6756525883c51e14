// IC-Light's "Lighting Preference" start (gradio_demo_iclight.py:235-299: bg_source, lowres_denoise, the img2img call), gfx950:
//   * the left / right / top / bottom light gradient as the [0,1]-convention image the VAE encoder takes;
//   * the img2img start latents  x_start = alpha*x0 + sigma_t*z  of the first executed sigma (diffusers' add_noise);
//   * for the background-conditioned model (generation.iclight_model: fbc): the background ramps of bg_source and the foreground's grey matte.
// Both run once per relight, in front of the denoise loop; every rounding is spelled out because the tests ask for the bits numpy gives.
#include "common.h"
#include "../../include/tclight_hip.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// np.linspace(start, stop, n)[k] in f64: start + k*step with step = (stop - start)/(n - 1), product and sum rounded on their own, the last
// sample set to `stop`; n == 1 gives `start`.  astype(uint8) truncates (the values lie in [0, 255]); the demo's numpy2pytorch feeds the
// VAE u/127 - 1, and VAEEngine.encode computes 2x - 1, so x = u/254 (one IEEE f32 division).
__device__ __forceinline__ float light_sample(int k, int n, double start, double stop, double step) {
#pragma clang fp contract(off)
    double v = start;
    if (n > 1) {
        const double kv = (double)k * step;
        v = k == n - 1 ? stop : kv + start;
    }
    const int u = (int)v;
    return (float)u / 254.f;
}

// out [3,H,W] f32, the same plane three times.  One lane per 4 consecutive floats of the flat [3*H*W] array (the allocation's start is 16 B
// aligned, a plane's need not be): full groups leave as one 16 B store, the last group element by element.
// The ramp runs from `start` at index 0 to `stop` at the last index of the axis `side` names (x for LEFT / RIGHT, y for TOP / BOTTOM).
__global__ __launch_bounds__(256) void k_light_gradient(float* __restrict__ out, int H, int W, int side, double start, double stop) {
    const int hw = H * W, total = 3 * hw, groups = (total + 3) / 4;          // the host refuses 3*H*W + 3 >= 2^31
    const bool horizontal = side == TCL_LIGHT_LEFT || side == TCL_LIGHT_RIGHT;
    const int n = horizontal ? W : H;
    const double step = n > 1 ? (stop - start) / (double)(n - 1) : 0.0;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {      // grid * 256 <= 2^23: no overflow
        const int e0 = g * 4;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + j < total ? e0 + j : total - 1;
            const int p = e % hw;
            v[j] = light_sample(horizontal ? p % W : p / W, n, start, stop, step);
        }
        if (e0 + 4 <= total) {
            *(float4*)(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int j = 0; j < 4 && e0 + j < total; ++j) out[e0 + j] = v[j];
        }
    }
}

// out[n][i] = f16(fl32(fl32(alpha*x0[n*x0_stride + i]) + fl32(sigma_t*z[n*z_stride + i]))), i < chw: no contraction, one rounding to f16.
// VEC: chw and both strides are multiples of 8 and the three bases 16 B aligned -> a lane owns 8 consecutive elements of one frame: one 16 B
// load of x0, two of z, one 16 B store.  Otherwise one element per lane.
template <bool VEC>
__global__ __launch_bounds__(256) void k_light_start(_Float16* __restrict__ out, const _Float16* __restrict__ x0, long x0_stride,
                                                     const float* __restrict__ z, long z_stride, long N, long chw, float alpha, float sigma_t) {
#pragma clang fp contract(off)
    constexpr int V = VEC ? 8 : 1;
    const long per = chw / V, total = N * per;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const long n = g / per, i = (g - n * per) * V;
        const _Float16* px = x0 + n * x0_stride + i;
        const float* pz = z + n * z_stride + i;
        _Float16* po = out + n * chw + i;
        if (VEC) {
            const h8 xv = *(const h8*)px;
            const float4 z0 = *(const float4*)pz, z1 = *(const float4*)(pz + 4);
            const float zv[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
            h8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float a = alpha * (float)xv[j], b = sigma_t * zv[j];
                const float s = a + b;
                o[j] = (_Float16)s;
            }
            *(h8*)po = o;
        } else {
            const float a = alpha * (float)*px, b = sigma_t * *pz;
            const float s = a + b;
            *po = (_Float16)s;
        }
    }
}

// IC-Light's background demo mattes the foreground onto 127-grey before the VAE sees it (run_rmbg: 127 + (img - 127) * alpha, clipped to uint8).
// frames [n,3,hw] f32 in [0,1], alpha [n,1,hw] f32: u = fl32(255 f); v = fl32(127 + fl32(fl32(u - 127) a)); q = trunc(clamp(v, 0, 255)), NaN -> 0;
// out = q/254 (the u/254 convention of light_sample).  A lane owns V consecutive pixels of one frame: one alpha load serves the three planes.
__device__ __forceinline__ float matte_sample(float f, float a) {
#pragma clang fp contract(off)
    const float u = 255.f * f;
    const float d = u - 127.f;
    const float m = d * a;
    const float v = 127.f + m;
    const float q = truncf(fminf(fmaxf(v, 0.f), 255.f));
    return q / 254.f;
}
template <bool VEC>
__global__ __launch_bounds__(256) void k_matte_grey(const float* __restrict__ frames, const float* __restrict__ alpha, float* __restrict__ out,
                                                    long n, long hw) {
    constexpr int V = VEC ? 4 : 1;
    const long per = hw / V, total = n * per;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const long f = g / per, i = (g - f * per) * V;
        const float* pa = alpha + f * hw + i;
        if (VEC) {
            const float4 a = *(const float4*)pa;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 x = *(const float4*)(frames + (f * 3 + c) * hw + i);
                *(float4*)(out + (f * 3 + c) * hw + i) = make_float4(matte_sample(x.x, a.x), matte_sample(x.y, a.y), matte_sample(x.z, a.z),
                                                                     matte_sample(x.w, a.w));
            }
        } else {
            const float a = *pa;
            for (int c = 0; c < 3; ++c) out[(f * 3 + c) * hw + i] = matte_sample(frames[(f * 3 + c) * hw + i], a);
        }
    }
}

extern "C" {

int tcl_light_gradient_f32(float* out, int H, int W, int side, hipStream_t st) {
    TCL_CHECK_ARG(out && H > 0 && W > 0 && side >= TCL_LIGHT_LEFT && side <= TCL_LIGHT_BOTTOM && ((uintptr_t)out & 15) == 0);
    TCL_CHECK_ARG(3L * H * W + 3 < (1L << 31));
    const long groups = (3L * H * W + 3) / 4;
    const double start = (side == TCL_LIGHT_LEFT || side == TCL_LIGHT_TOP) ? 255.0 : 0.0;
    hipLaunchKernelGGL(k_light_gradient, dim3(stream_grid(groups, 256, 1)), dim3(256), 0, st, out, H, W, side, start, 255.0 - start);
    TCL_LAUNCH_RET();
}

int tcl_bg_ramp_f32(float* out, int H, int W, int side, int start, int stop, hipStream_t st) {
    TCL_CHECK_ARG(out && H > 0 && W > 0 && side >= TCL_LIGHT_LEFT && side <= TCL_LIGHT_BOTTOM && ((uintptr_t)out & 15) == 0);
    TCL_CHECK_ARG(start >= 0 && start <= 255 && stop >= 0 && stop <= 255 && 3L * H * W + 3 < (1L << 31));
    const long groups = (3L * H * W + 3) / 4;
    hipLaunchKernelGGL(k_light_gradient, dim3(stream_grid(groups, 256, 1)), dim3(256), 0, st, out, H, W, side, (double)start, (double)stop);
    TCL_LAUNCH_RET();
}

int tcl_matte_grey_f32(const float* frames, const float* alpha, float* out, int n, int H, int W, hipStream_t st) {
    TCL_CHECK_ARG(frames && alpha && out && n > 0 && H > 0 && W > 0);
    const long hw = (long)H * W;
    const bool vec = hw % 4 == 0 && (((uintptr_t)frames | (uintptr_t)alpha | (uintptr_t)out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(k_matte_grey<true>, dim3(stream_grid(n * (hw / 4), 256, 1)), dim3(256), 0, st, frames, alpha, out, (long)n, hw);
    else
        hipLaunchKernelGGL(k_matte_grey<false>, dim3(stream_grid(n * hw, 256, 1)), dim3(256), 0, st, frames, alpha, out, (long)n, hw);
    TCL_LAUNCH_RET();
}

int tcl_light_start_f16(void* out, const void* x0, long x0_stride, const float* z, long z_stride, int N, long chw, float alpha, float sigma_t,
                        hipStream_t st) {
    TCL_CHECK_ARG(out && x0 && z && N > 0 && chw > 0);
    TCL_CHECK_ARG((x0_stride == 0 || x0_stride >= chw) && (z_stride == 0 || z_stride >= chw));
    const bool vec = chw % 8 == 0 && x0_stride % 8 == 0 && z_stride % 8 == 0 &&
                     (((uintptr_t)out | (uintptr_t)x0 | (uintptr_t)z) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(k_light_start<true>, dim3(stream_grid((long)N * (chw / 8), 256, 1)), dim3(256), 0, st, (_Float16*)out, (const _Float16*)x0,
                           x0_stride, z, z_stride, (long)N, chw, alpha, sigma_t);
    else
        hipLaunchKernelGGL(k_light_start<false>, dim3(stream_grid((long)N * chw, 256, 1)), dim3(256), 0, st, (_Float16*)out, (const _Float16*)x0,
                           x0_stride, z, z_stride, (long)N, chw, alpha, sigma_t);
    TCL_LAUNCH_RET();
}

}  // extern "C"
