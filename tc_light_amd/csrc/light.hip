// IC-Light's "Lighting Preference" start (gradio_demo_iclight.py:235-299: bg_source, lowres_denoise, the img2img call), gfx950:
//   * the left / right / top / bottom light gradient as the [0,1]-convention image the VAE encoder takes;
//   * the img2img start latents  x_start = alpha*x0 + sigma_t*z  of the first executed sigma (diffusers' add_noise);
//   * for the background-conditioned model (generation.iclight_model: fbc): the background ramps of bg_source and the foreground's grey matte;
//   * for generation.normal (the background demo's "Compute Normal", process_normal): the matte with its sigma offset and the kernel that turns the
//     four directional relights into a surface normal and the ambient image;
//   * for generation.light_path (an animated light): one ramp per frame at an arbitrary angle.
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

// generation.light_path: the ramp of one frame at an arbitrary angle.  (c, s) is the frame's unit vector, R the half extent of the image along it;
// every operation in f64 and rounded on its own, the division IEEE: d = px*c + py*s; t = (R - d)/(2R), t0 when R == 0; v = lo + (hi - lo)*t;
// u = trunc(clamp(v, 0, 255)); out = u/254 as light_sample stores it.
// R == 0: the image has a single sample along the light's axis.  np.linspace(start, stop, 1) keeps the FIRST sample, so the pixel counts as the
// origin corner of a square image, whose t is t0 = ((|c| + |s|) + (c + s)) / (2(|c| + |s|)): exactly 1 at 0 / 90, 0 at 180 / 270 -- the level
// tcl_light_gradient_f32 / tcl_bg_ramp_f32 give at n == 1 -- and continuous in the angle between them.
__device__ __forceinline__ float ramp_angle_sample(double px, double py, double c, double s, double R, double t0, double hi, double lo) {
#pragma clang fp contract(off)
    const double a = px * c, b = py * s;
    const double d = a + b;
    double t = t0;
    if (R != 0.0) {
        const double num = R - d, den = 2.0 * R;
        t = num / den;
    }
    const double w = (hi - lo) * t;
    const double v = lo + w;
    const int u = (int)trunc(fmin(fmax(v, 0.0), 255.0));       // NaN -> 0
    return (float)u / 254.f;
}

// out [N,3,hw] f32, dir [N,2] f64.  HBM-write-bound (12 B per pixel out, nothing in but the frame's pair).  VEC: hw % 4 == 0 and out 16 B aligned -> a
// lane owns 4 consecutive pixels of one frame, computes each once and stores one float4 to each of the three planes.  Otherwise one pixel per lane.
template <bool VEC>
__global__ __launch_bounds__(256) void k_light_ramp_angle(float* __restrict__ out, const double* __restrict__ dir, long N, int H, int W, double hi,
                                                          double lo) {
#pragma clang fp contract(off)
    constexpr int V = VEC ? 4 : 1;
    const long hw = (long)H * W, per = hw / V, total = N * per;
    const double cx = (double)(W - 1) / 2.0, cy = (double)(H - 1) / 2.0;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const long f = g / per;
        const int p = (int)(g - f * per) * V;
        const double c = dir[2 * f], s = dir[2 * f + 1];
        const double ex = fabs(c) * (double)(W - 1), ey = fabs(s) * (double)(H - 1);
        const double R = (ex + ey) / 2.0;
        double t0 = 0.5;
        if (R == 0.0) {
            const double A = fabs(c) + fabs(s), cs = c + s;
            const double num = A + cs, den = 2.0 * A;
            t0 = num / den;
        }
        int y = p / W, x = p - y * W;
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            v[j] = ramp_angle_sample((double)x - cx, (double)y - cy, c, s, R, t0, hi, lo);
            if (++x == W) { x = 0; ++y; }
        }
        float* po = out + f * 3 * hw + p;
        if constexpr (VEC) {
            const float4 q = make_float4(v[0], v[1], v[2], v[3]);
#pragma unroll
            for (int k = 0; k < 3; ++k) *(float4*)(po + k * hw) = q;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) po[k * hw] = v[0];
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
// sigma: process_normal's run_rmbg(img, sigma=16) adds it to (u - 127) before the alpha; (u - 127) + 0 is exact, so sigma = 0 is the plain matte.
__device__ __forceinline__ float matte_sample(float f, float a, float sigma) {
#pragma clang fp contract(off)
    const float u = 255.f * f;
    const float d = (u - 127.f) + sigma;
    const float m = d * a;
    const float v = 127.f + m;
    const float q = truncf(fminf(fmaxf(v, 0.f), 255.f));
    return q / 254.f;
}
template <bool VEC>
__global__ __launch_bounds__(256) void k_matte_grey(const float* __restrict__ frames, const float* __restrict__ alpha, float* __restrict__ out,
                                                    long n, long hw, float sigma) {
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
                *(float4*)(out + (f * 3 + c) * hw + i) = make_float4(matte_sample(x.x, a.x, sigma), matte_sample(x.y, a.y, sigma),
                                                                     matte_sample(x.z, a.z, sigma), matte_sample(x.w, a.w, sigma));
            }
        } else {
            const float a = *pa;
            for (int c = 0; c < 3; ++c) out[(f * 3 + c) * hw + i] = matte_sample(frames[(f * 3 + c) * hw + i], a, sigma);
        }
    }
}

// process_normal of IC-Light's background demo on the four decoded relights of one pixel (left, right, bottom, top; 3 channels each) and its matting
// alpha.  Every operation in f32, rounded on its own.  The inputs are clamped to [0,1] (NaN -> 0), so each is at most 4A and q lies in [-1, 3];
// u^2 + v^2 + h^2 >= 0.30 (h = (1 - u^2 - v^2)^5 where that is positive), so neither division meets a zero and finite input gives finite output.
struct NormalPx { float n[3]; float amb[3]; };
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }      // NaN -> 0
__device__ __forceinline__ NormalPx normal_sample(const float l[3], const float r[3], const float b[3], const float t[3], float a) {
#pragma clang fp contract(off)
    const float e = 1e-5f;
    NormalPx o;
    float uc[3], vc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float L = clamp01(l[c]), R = clamp01(r[c]), B = clamp01(b[c]), T = clamp01(t[c]);
        const float A = (((L + R) + B) + T) * 0.25f;
        const float den = A + e;
        const float ql = (L + e) / den - 1.f, qr = (R + e) / den - 1.f, qb = (B + e) / den - 1.f, qt = (T + e) / den - 1.f;
        uc[c] = (qr - ql) * 0.5f;
        vc[c] = (qt - qb) * 0.5f;
        o.amb[c] = A;
    }
    const float u = ((uc[0] + uc[1]) + uc[2]) / 3.f, v = ((vc[0] + vc[1]) + vc[2]) / 3.f;
    const float uu = u * u, vv = v * v;
    const float s = fminf(fmaxf((1.f - uu) - vv, 0.f), 1e5f);
    const float s2 = s * s, s4 = s2 * s2, h = s4 * s;          // the demo's ** (0.5 * sigma), sigma = 10
    const float len = sqrtf((uu + vv) + h * h);
    const float m = truncf(fminf(fmaxf(a * 255.f, 0.f), 255.f)) / 255.f;      // the demo's u8 round trip of the matte; NaN -> 0
    const float k = 1.f - m;
    o.n[0] = (u / len) * m + 0.f * k;                          // the (0, 0, 1) of the blend: -0 becomes +0, as in the stated formula
    o.n[1] = (v / len) * m + 0.f * k;
    o.n[2] = (h / len) * m + k;
    return o;
}
__device__ __forceinline__ unsigned normal_quant(float x) {
#pragma clang fp contract(off)
    const float y = x * 127.5f;
    return (unsigned)truncf(fminf(fmaxf(y + 127.5f, 0.f), 255.f));
}

// left / right / bottom / top [n,3,hw] f32, alpha [n,1,hw] f32 or NULL (= 1) -> nu8 [n,hw,3] u8, nf32 / amb [n,3,hw] f32 (either may be NULL).
// HBM-bound (52 B in, up to 27 B out per pixel).  A lane owns 4 consecutive pixels of one frame and issues its 13 loads before the first operation
// on them.  VEC: hw % 4 == 0 and every pointer aligned -> 16 B loads, the 12 u8 as three dwords, 16 B stores of the f32 planes.  Otherwise dword loads at
// indices clamped to the frame (a lane of the last group loads the last pixel again, and stores only its own).  ALPHA: false = no matte, alpha is 1.
template <bool VEC, bool ALPHA>
__global__ __launch_bounds__(256) void k_fbc_normal(const float* __restrict__ left, const float* __restrict__ right, const float* __restrict__ bottom,
                                                    const float* __restrict__ top, const float* __restrict__ alpha, uint8_t* __restrict__ nu8,
                                                    float* __restrict__ nf32, float* __restrict__ amb, long n, long hw) {
    const long per = (hw + 3) / 4, total = n * per;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const long f = g / per, i = (g - f * per) * 4;
        const float* src[4] = {left, right, bottom, top};
        float x[4][3][4], a[4] = {1.f, 1.f, 1.f, 1.f};
        if (VEC) {
            if (ALPHA) {
                const float4 q = *(const float4*)(alpha + f * hw + i);
                a[0] = q.x; a[1] = q.y; a[2] = q.z; a[3] = q.w;
            }
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float4 q = *(const float4*)(src[d] + (f * 3 + c) * hw + i);
                    x[d][c][0] = q.x; x[d][c][1] = q.y; x[d][c][2] = q.z; x[d][c][3] = q.w;
                }
        } else {
            long p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = i + j < hw ? i + j : hw - 1;
            if (ALPHA) {
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = alpha[f * hw + p[j]];
            }
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j) x[d][c][j] = src[d][(f * 3 + c) * hw + p[j]];
        }
        __builtin_amdgcn_sched_barrier(0);      // nothing below is scheduled in front of a load: the scheduler otherwise trickles them in behind the divisions
        NormalPx o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float l[3], r[3], b[3], t[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { l[c] = x[0][c][j]; r[c] = x[1][c][j]; b[c] = x[2][c][j]; t[c] = x[3][c][j]; }
            o[j] = normal_sample(l, r, b, t, a[j]);
        }
        unsigned q[12];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) q[j * 3 + c] = normal_quant(o[j].n[c]);
        if (VEC) {
            unsigned* pu = (unsigned*)(nu8 + (f * hw + i) * 3);
#pragma unroll
            for (int w = 0; w < 3; ++w) pu[w] = q[4 * w] | (q[4 * w + 1] << 8) | (q[4 * w + 2] << 16) | (q[4 * w + 3] << 24);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (nf32) *(float4*)(nf32 + (f * 3 + c) * hw + i) = make_float4(o[0].n[c], o[1].n[c], o[2].n[c], o[3].n[c]);
                if (amb) *(float4*)(amb + (f * 3 + c) * hw + i) = make_float4(o[0].amb[c], o[1].amb[c], o[2].amb[c], o[3].amb[c]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i + j < hw) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        nu8[(f * hw + i + j) * 3 + c] = (uint8_t)q[j * 3 + c];
                        if (nf32) nf32[(f * 3 + c) * hw + i + j] = o[j].n[c];
                        if (amb) amb[(f * 3 + c) * hw + i + j] = o[j].amb[c];
                    }
                }
            }
        }
    }
}

extern "C" {

int tcl_fbc_normal(const float* left, const float* right, const float* bottom, const float* top, const float* alpha, void* normal_u8,
                   float* normal_f32, float* ambient, int n, int H, int W, hipStream_t st) {
    TCL_CHECK_ARG(left && right && bottom && top && normal_u8 && n > 0 && H > 0 && W > 0);
    TCL_CHECK_ARG(3L * n * H * W < (1L << 31));
    const long hw = (long)H * W;
    const uintptr_t p16 = (uintptr_t)left | (uintptr_t)right | (uintptr_t)bottom | (uintptr_t)top | (uintptr_t)alpha | (uintptr_t)normal_f32 |
                          (uintptr_t)ambient;      // a null optional pointer adds no bit
    const bool vec = hw % 4 == 0 && (p16 & 15) == 0 && ((uintptr_t)normal_u8 & 3) == 0;
    const int grid = stream_grid(n * ((hw + 3) / 4), 256, 1);
    auto k = vec ? (alpha ? k_fbc_normal<true, true> : k_fbc_normal<true, false>) : (alpha ? k_fbc_normal<false, true> : k_fbc_normal<false, false>);
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, st, left, right, bottom, top, alpha, (uint8_t*)normal_u8, normal_f32, ambient, (long)n, hw);
    TCL_LAUNCH_RET();
}

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

int tcl_light_ramp_angle_f32(float* out, const double* dir, int N, int H, int W, int hi, int lo, hipStream_t st) {
    TCL_CHECK_ARG(out && dir && N > 0 && H > 0 && W > 0);
    TCL_CHECK_ARG(3L * N * H * W < (1L << 31));
    TCL_CHECK_ARG(hi >= 0 && hi <= 255 && lo >= 0 && lo <= 255 && hi >= lo);
    const long hw = (long)H * W;
    if (hw % 4 == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL(k_light_ramp_angle<true>, dim3(stream_grid(N * (hw / 4), 256, 1)), dim3(256), 0, st, out, dir, (long)N, H, W, (double)hi,
                           (double)lo);
    else
        hipLaunchKernelGGL(k_light_ramp_angle<false>, dim3(stream_grid(N * hw, 256, 1)), dim3(256), 0, st, out, dir, (long)N, H, W, (double)hi,
                           (double)lo);
    TCL_LAUNCH_RET();
}

int tcl_matte_grey_sigma_f32(const float* frames, const float* alpha, float* out, int n, int H, int W, float sigma, hipStream_t st) {
    TCL_CHECK_ARG(frames && alpha && out && n > 0 && H > 0 && W > 0 && sigma == sigma);
    const long hw = (long)H * W;
    const bool vec = hw % 4 == 0 && (((uintptr_t)frames | (uintptr_t)alpha | (uintptr_t)out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(k_matte_grey<true>, dim3(stream_grid(n * (hw / 4), 256, 1)), dim3(256), 0, st, frames, alpha, out, (long)n, hw, sigma);
    else
        hipLaunchKernelGGL(k_matte_grey<false>, dim3(stream_grid(n * hw, 256, 1)), dim3(256), 0, st, frames, alpha, out, (long)n, hw, sigma);
    TCL_LAUNCH_RET();
}

int tcl_matte_grey_f32(const float* frames, const float* alpha, float* out, int n, int H, int W, hipStream_t st) {
    return tcl_matte_grey_sigma_f32(frames, alpha, out, n, H, W, 0.f, st);
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
