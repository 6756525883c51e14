"""References for DDIM inversion on the IC-Light UNet (tc_light_amd/invert.py), restated here from the published algorithm (the reference's
`Inverter.pred_next_x`, `ddim_inversion`, `ddim_sample`): no GPU, no engine code.

  ddim_coeffs     the four scalars of every level, float64
  ddim_step_ref   one update in numpy float32 with the kernel's operation order (every product, difference, quotient and sum rounded on its own)
  ddim_step_f64   the direct float64 transliteration of pred_next_x
  step_bound      the worst-case distance of the two, from the f32 roundings (derivation below); roundtrip_bound: inversion followed by sampling
  invert_ref / sample_ref   the loops over oracle.sd15.unet_forward (VidToMe off), f32 master latents; half=True: the oracle's f16-output mode
"""
import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of float32 (round to nearest)


def sd15_alphas_cumprod():
    """SD-1.5's training schedule as init_iclight builds it: 1000 linear betas 0.00085 .. 0.012 (f32), cumulative product in float64."""
    betas = np.linspace(0.00085, 0.012, 1000, dtype=np.float64).astype(np.float32)
    return np.cumprod(1.0 - betas.astype(np.float64))


def ddim_coeffs(alphas_cumprod, timesteps):
    """timesteps strictly ascending -> [(mu, sigma, mu_prev, sigma_prev)] float64 per level; `prev` of level i is level i-1 and
    final_alpha_cumprod = alphas_cumprod[0] (set_alpha_to_one: false) below the first level."""
    ac = np.asarray(alphas_cumprod, np.float64)
    out = []
    for i, t in enumerate(timesteps):
        a_t, a_p = ac[int(t)], (ac[int(timesteps[i - 1])] if i > 0 else ac[0])
        out.append((float(np.sqrt(a_t)), float(np.sqrt(1.0 - a_t)), float(np.sqrt(a_p)), float(np.sqrt(1.0 - a_p))))
    return out


def _ab(coeffs, inversion, dtype):
    mu, sigma, mu_prev, sigma_prev = (dtype(c) for c in coeffs)
    return (sigma_prev, mu_prev, mu, sigma) if inversion else (sigma, mu, mu_prev, sigma_prev)       # s_a, m_a, m_b, s_b


def ddim_step_ref(x, eps, coeffs, inversion):
    """x, eps float32 arrays (eps holds f16 values) -> x_new float32:  x0 = (x - s_a*eps) / m_a;  x = m_b*x0 + s_b*eps."""
    x, eps = np.asarray(x, np.float32), np.asarray(eps, np.float32)
    s_a, m_a, m_b, s_b = _ab(coeffs, inversion, np.float32)
    se = (s_a * eps).astype(np.float32)
    x0 = ((x - se).astype(np.float32) / m_a).astype(np.float32)
    a, b = (m_b * x0).astype(np.float32), (s_b * eps).astype(np.float32)
    return (a + b).astype(np.float32)


def ddim_step_f64(x, eps, coeffs, inversion):
    """pred_next_x as written, in float64."""
    x, eps = np.asarray(x, np.float64), np.asarray(eps, np.float64)
    mu, sigma, mu_prev, sigma_prev = coeffs
    if inversion:
        pred_x0 = (x - sigma_prev * eps) / mu_prev
        return mu * pred_x0 + sigma * eps
    pred_x0 = (x - sigma * eps) / mu
    return mu_prev * pred_x0 + sigma_prev * eps


def step_bound(x, eps, coeffs, inversion):
    """|ddim_step_ref - ddim_step_f64| <= this, per element.  With u = 2^-24 and A = (|x| + |s_a eps|) / m_a (the magnitude that enters x0):
      x0:  s_a and m_a rounded to f32 (u |s_a eps| / m_a, u |x0|), the product, the difference and the quotient rounded (u |s_a eps| / m_a, u |d| / m_a,
           u |x0|), each <= u A                                                                                        -> 5 u A
      m_b*x0: m_b rounded, the product rounded, the error of x0 carried                                               -> (2 + 5) u m_b A
      s_b*eps: s_b rounded, the product rounded                                                                        -> 2 u |s_b eps|
      the sum rounded: u (|a| + |b|) <= u (m_b A + |s_b eps|)
    total 8 u m_b A + 3 u |s_b eps|: a few f32 ulps of the result's magnitude; 1 % on top for the second-order terms."""
    x, eps = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(eps, np.float64))
    s_a, m_a, m_b, s_b = _ab(coeffs, inversion, np.float64)
    A = (x + s_a * eps) / m_a
    return 1.01 * U32 * (8.0 * m_b * A + 3.0 * s_b * eps)


def roundtrip_bound(x, eps, coeffs):
    """Inversion to x1 followed by sampling with the same eps and coefficients returns x exactly in real arithmetic; in f32 the first step's error E1
    passes through x0' = (x1 - sigma eps) / mu and x' = mu_prev x0' (factor mu_prev / mu) and the second step adds its own E2 (taken at x1)."""
    mu, _, mu_prev, _ = coeffs
    x1 = ddim_step_f64(x, eps, coeffs, True)
    return (mu_prev / mu) * step_bound(x, eps, coeffs, True) + step_bound(x1, eps, coeffs, False)


def _eps(sd, x, cc, t, text, half):
    from oracle import sd15 as OS
    n = x.shape[0]
    xi = x.half().float() if half else x                      # an f16 pipeline feeds the UNet f16 latents; the master stays f32 either way
    sample = torch.cat([xi, cc], dim=1)
    if n % 2:                                                 # unet_forward takes a pair batch [2F, ...]: rows are independent (no merging)
        sample = torch.cat([sample, sample[-1:]])
    with torch.no_grad():
        if half:
            with OS.half_outputs():
                e = OS.unet_forward(sd, sample, float(t), text, tome=None)
        else:
            e = OS.unet_forward(sd, sample, float(t), text, tome=None)
    return e[:n]


def _loop(sd, x, cc, text, alphas_cumprod, timesteps, levels, inversion, half):
    alphas_cumprod = sd15_alphas_cumprod() if alphas_cumprod is None else alphas_cumprod
    coeffs = ddim_coeffs(alphas_cumprod, timesteps)
    x = x.float().clone()
    for i in levels:
        e = _eps(sd, x, cc.float(), timesteps[i], text.float(), half)
        x = torch.from_numpy(ddim_step_ref(x.numpy(), e.numpy(), coeffs[i], inversion))
    return x


def invert_ref(sd, frames_latents, cond_latents, text, timesteps, half=False, alphas_cumprod=None):
    """Clean latents [N,4,h,w] -> latents at timesteps[-1]; timesteps strictly ascending; text [2,L,768] with both halves the same condition.
    eps is predicted at the level being stepped to."""
    return _loop(sd, frames_latents, cond_latents, text, alphas_cumprod, timesteps, range(len(timesteps)), True, half)


def sample_ref(sd, noisy_latents, cond_latents, text, timesteps, half=False, alphas_cumprod=None):
    """Deterministic DDIM sampling from timesteps[-1] back down the same levels."""
    return _loop(sd, noisy_latents, cond_latents, text, alphas_cumprod, timesteps, range(len(timesteps) - 1, -1, -1), False, half)
