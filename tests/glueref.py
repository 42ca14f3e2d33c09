"""CPU references of the glue kernels in csrc/elementwise.hip (scheduler step, UNet-input pack, posterior sample,
latents -> VAE, image <-> tensor).  No GPU import.

The fp32 ones restate a kernel operation for operation, in its order, in NumPy float32 (every NumPy float32 operation
rounds once, so there is no FMA): the kernels are compiled with -ffp-contract=off and claim the same bits.  Storage
rounding to a 16-bit type is left to the caller: `torch.from_numpy(ref).to(dtype)` is round-to-nearest-even, as
`from_f<T>` is.  `latent_sample_f64` is the one float64 reference (expf is not bit-reproducible), returned with
the per-element rounding budget to compare under.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

f32 = np.float32


class StepOut(NamedTuple):
    x: np.ndarray                      # x_out: the new latents
    eps: np.ndarray                    # the CFG-combined eps (what hist_store receives when the plan stores it)
    cur: Optional[np.ndarray]          # what cur_store receives (the step's source sample), None if not saved
    unet_in: Optional[np.ndarray]      # fp32 [(2)B, h, w, cin_pad] packed next UNet input, None without cin_pad


def pack_unet_input(lat, cfg, cin_pad, mask=None, masked=None):
    """pack_kernel / pack_pixel: [lat4 | mask, masked4 | 0...] per pixel, fp32 [(2 if cfg else 1) * B, h, w, cin_pad];
    both CFG halves are the same.  lat, masked: [B, h, w, 4]; mask: [B, h, w]."""
    B, h, w, _ = lat.shape
    out = np.zeros((B, h, w, cin_pad), dtype=f32)
    out[..., :4] = lat
    if mask is not None:
        out[..., 4] = mask
        out[..., 5:9] = masked
    return np.concatenate([out, out]) if cfg else out


def emulate_step(plan, eps_u, eps_c, guidance, x, slots, cur, cin_pad=None, mask=None, masked=None) -> StepOut:
    """float32 restatement of step_kernel (csrc/elementwise.hip) for one plan.  `slots` (list) and `cur` (1-list)
    are the history state and are updated as the kernel updates hist_store / cur_store."""
    f = f32
    e0 = (eps_u + f(guidance) * (eps_c - eps_u)) if eps_c is not None else eps_u
    if plan.store_slot is not None:
        slots[plan.store_slot] = e0.copy()
    e = f(plan.hw[0]) * e0
    for k in range(4):
        if plan.hist[k] is not None:
            e = e + f(plan.hw[k + 1]) * slots[plan.hist[k]]
    e = e / f(plan.e_div)
    e = f(plan.e_mul) * e
    xs = cur[0] if plan.x_from_cur else x
    saved = None
    if plan.save_cur:
        cur[0] = xs.copy()
        saved = cur[0]
    c0, c1, c2, c3 = (f(v) for v in plan.c)
    if plan.mode == 0:
        r = c0 * xs - (c1 * e) / c2
    else:
        x0 = (xs - c0 * e) / c1
        r = c2 * x0 + c3 * e
    packed = None if cin_pad is None else pack_unet_input(r, eps_c is not None, cin_pad, mask, masked)
    return StepOut(r, e0, saved, packed)


def image_to_tensor(img_u8, cpad, mask=None):
    """img2t_kernel: uint8 [B, H, W, 3] -> fp32 [B, H, W, cpad]; u8 / 255, then 2x - 1, then * (mask < 0.5)."""
    v = img_u8.astype(f32) / f32(255.0)
    v = f32(2.0) * v - f32(1.0)
    if mask is not None:
        v = v * np.where(mask < f32(0.5), f32(1.0), f32(0.0))[..., None]
    out = np.zeros(img_u8.shape[:3] + (cpad,), dtype=f32)
    out[..., :3] = v
    return out


def tensor_to_image(x):
    """t2img_kernel on the fp32 value of the stored input, x [..., >= 3]: (uint8 [..., 3], f01 fp32 [..., 3]).
    x * 0.5 + 0.5, clamp to [0, 1], * 255, round half to even."""
    v = x[..., :3].astype(f32) * f32(0.5) + f32(0.5)
    v = np.minimum(np.maximum(v, f32(0.0)), f32(1.0))
    return np.rint(v * f32(255.0)).astype(np.uint8), v


def t2img_fp32_grid():
    """fp32 inputs of t2img around every rounding boundary: for each k in 0..254 the x nearest 2 (k + 0.5) / 255 - 1
    and its 8 neighbours on either side, which include every x whose fp32 product v * 255 lands exactly on k + 0.5 (a
    tie for rintf, although (k + 0.5) / 255 itself is an fp32 number only at k = 127); then the clamp: values below
    -1 and above 1, +-1, +-0.  A multiple of 3 values, flat."""
    k = np.arange(255, dtype=np.float64)
    x = ((2.0 * (k + 0.5) / 255.0) - 1.0).astype(f32)
    lo, hi = x.copy(), x.copy()
    near = [x]
    for _ in range(8):
        lo, hi = np.nextafter(lo, f32(-2.0)), np.nextafter(hi, f32(2.0))
        near += [lo, hi]
    edge = np.array([-3.0e38, -1.0e4, -1.5, -1.0000001, -1.0, -0.99999994, -0.0, 0.0, 0.99999994, 1.0, 1.0000001, 1.5,
                     1.0e4, 3.0e38], dtype=f32)
    g = np.concatenate(near + [edge, np.linspace(-1.25, 1.25, 1001, dtype=f32)])
    return np.concatenate([g, np.zeros(-g.size % 3, dtype=f32)])


def latents_to_vae(lat, sf):
    """scale_copy_kernel as irx_latents_to_vae runs it: fp32 [B, h, w, 8] = [lat / sf | 0, 0, 0, 0]."""
    out = np.zeros(lat.shape[:3] + (8,), dtype=f32)
    out[..., :4] = lat / f32(sf)
    return out


# |got - ref| <= 8 * 2^-24 * (|a| |sf| (|mean| + std |eps|) + |b noise|): about six fp32 roundings (0.5 * logvar, the
# product with eps, the sum, sf *, a *, b *, the final sum) of half an ulp each, plus a 1-ulp expf
LATENT_BOUND_ULPS = 8.0


def _bcast(t, B, bcast):
    """eps / noise as latent_kernel indexes them: one [h, w, 4] image for every batch entry, or one per entry."""
    return np.broadcast_to(t, (B,) + t.shape) if bcast else t


def latent_sample_f64(mom, eps, noise, bcast, sf, a, b):
    """float64 reference of latent_kernel on the moments as stored (mom [B, h, w, 8], already rounded to the storage
    type, any float dtype): (value, rounding budget), both float64 [B, h, w, 4].  sf, a, b are the fp32 scalars the
    kernel receives.  eps / noise: [h, w, 4] with bcast, [B, h, w, 4] without."""
    mom = mom.astype(np.float64)
    B = mom.shape[0]
    sf, a, b = (float(f32(v)) for v in (sf, a, b))
    mean, logvar = mom[..., :4], mom[..., 4:8]
    std = np.exp(0.5 * np.clip(logvar, -30.0, 20.0))
    e = _bcast(eps.astype(np.float64), B, bcast)
    z = sf * (mean + std * e)
    mag = abs(sf) * (np.abs(mean) + std * np.abs(e))
    if noise is not None:
        n = _bcast(noise.astype(np.float64), B, bcast)
        z = a * z + b * n
        mag = abs(a) * mag + np.abs(b * n)
    return z, LATENT_BOUND_ULPS * 2.0 ** -24 * mag


def latent_sample_f32(mom, eps, noise, bcast, sf, a, b):
    """torch CPU fp32 restatement of latent_kernel (torch.exp for expf), fp32 [B, h, w, 4] as a NumPy array."""
    import torch
    mom = torch.from_numpy(np.ascontiguousarray(mom.astype(f32)))
    B = mom.shape[0]
    sf, a, b = (float(f32(v)) for v in (sf, a, b))          # python scalars: the tensors stay fp32
    mean, logvar = mom[..., :4], mom[..., 4:8]
    logvar = torch.clamp(logvar, -30.0, 20.0)
    std = torch.exp(0.5 * logvar)
    z = mean + std * torch.from_numpy(np.array(_bcast(eps, B, bcast)))
    z = sf * z
    if noise is not None:
        z = a * z + b * torch.from_numpy(np.array(_bcast(noise, B, bcast)))
    assert z.dtype == torch.float32
    return z.numpy()


def latent_case(torch_dtype, B, h, w, bcast, with_noise, seed=0):
    """Inputs of one latent_sample case: moments rounded to the storage type (a torch CPU tensor, [B, h, w, 8]) with
    logvar entries on both sides of, and on, the clamp (-40, -30, 0, 20, 25) among random ones; fp32 eps / noise."""
    import torch
    rng = np.random.default_rng(seed)
    mom = rng.standard_normal((B, h, w, 8)).astype(f32)
    mom[..., 4:] *= f32(4.0)
    lv = mom[..., 4:].reshape(-1)
    edge = np.array([-40.0, -30.0, 0.0, 20.0, 25.0], dtype=f32)
    at = rng.permutation(lv.size)[:3 * edge.size]
    lv[at] = np.tile(edge, 3)
    mom[..., 4:] = lv.reshape(B, h, w, 4)
    shape = (h, w, 4) if bcast else (B, h, w, 4)
    eps = rng.standard_normal(shape).astype(f32)
    noise = rng.standard_normal(shape).astype(f32) if with_noise else None
    return torch.from_numpy(mom).to(torch_dtype), eps, noise
