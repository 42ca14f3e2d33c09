"""CPU tests of the glue-kernel references in tests/glueref.py: the references against the oracle's own image
processing, and the rounding budget of the posterior-sample check (tests/test_glue_gpu.py holds the kernel to the
same budget) on a torch fp32 restatement of the kernel."""
import numpy as np
import pytest
import torch

from image_restoration_and_enhancement_amd import schedulers as S
from image_restoration_and_enhancement_amd.configs import SchedulerConfig
from oracle import pipeline_ref as PR
from tests import glueref as G

SF = 0.18215


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bcast", [0, 1])
@pytest.mark.parametrize("with_noise", [False, True])
def test_latent_sample_fp32_within_budget(dtype, bcast, with_noise):
    """The fp32 restatement of latent_kernel stays inside 8 * 2^-24 * (|a| |sf| (|mean| + std |eps|) + |b noise|) of
    float64 on the same rounded moments (measured worst case over these cases: 3.06 of the 8 units of 2^-24), so the
    bound the GPU test uses is one the arithmetic itself honours, with the margin the derivation leaves."""
    a, b = S.make_planner(SchedulerConfig(kind="ddim")).add_noise_coeffs(501) if with_noise else (1.0, 0.0)
    worst = 0.0
    for (B, h, w) in ((1, 5, 3), (3, 7, 13), (3, 32, 32)):
        mom, eps, noise = G.latent_case(dtype, B, h, w, bcast, with_noise)
        mom = mom.float().numpy()
        ref, budget = G.latent_sample_f64(mom, eps, noise, bcast, SF, a, b)
        got = G.latent_sample_f32(mom, eps, noise, bcast, SF, a, b).astype(np.float64)
        assert np.isfinite(got).all()
        err = np.abs(got - ref)
        worst = max(worst, float((err / np.maximum(budget, 1e-300)).max()) * G.LATENT_BOUND_ULPS)
        assert (err <= budget).all(), (B, h, w, worst)
    assert worst <= G.LATENT_BOUND_ULPS, worst


def test_latent_case_has_clamp_edges():
    mom, _, _ = G.latent_case(torch.bfloat16, 1, 5, 3, 1, False)
    lv = mom[..., 4:].float().reshape(-1).tolist()
    for v in (-40.0, -30.0, 0.0, 20.0, 25.0):
        assert v in lv


def test_latent_ref_is_the_oracle_formula():
    """float64 reference == diffusers' DiagonalGaussianDistribution.sample * sf, then add_noise (oracle)."""
    mom, eps, noise = G.latent_case(torch.float32, 2, 4, 4, 0, True)
    m = mom.double()
    ref = PR.DDIMRef()
    z = (m[..., :4] + torch.exp(0.5 * m[..., 4:].clamp(-30.0, 20.0)) * torch.from_numpy(eps).double()) \
        * float(np.float32(SF))
    a = ref.alphas_cumprod[501].double()
    want = np.sqrt(float(np.float32(a ** 0.5)) ** 2) * z + float(np.float32((1 - ref.alphas_cumprod[501]) ** 0.5)) \
        * torch.from_numpy(noise).double()
    a32, b32 = S.make_planner(SchedulerConfig(kind="ddim")).add_noise_coeffs(501)
    got, _ = G.latent_sample_f64(mom.numpy(), eps, noise, 0, SF, a32, b32)
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-12, atol=1e-12)


def test_image_refs_match_oracle_processing():
    """img2t == VaeImageProcessor.preprocess arithmetic (u8 / 255, 2x - 1, masked where mask >= 0.5); t2img ==
    postprocess (x / 2 + 0.5, clamp, * 255, numpy round half to even)."""
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (1, 8, 8, 3), dtype=np.uint8)
    mask = rng.choice(np.array([0, 0.49, 0.5, 1], dtype=np.float32), (1, 8, 8))
    t = 2.0 * torch.from_numpy(img.astype(np.float32) / 255.0) - 1.0
    got = G.image_to_tensor(img, 8)
    assert np.array_equal(got[..., :3], t.numpy()) and not got[..., 3:].any()
    gm = G.image_to_tensor(img, 3, mask)
    assert np.array_equal(gm, (t * (torch.from_numpy(mask) < 0.5)[..., None]).numpy())
    x = torch.from_numpy(np.linspace(-1.5, 1.5, 3 * 4001, dtype=np.float32).reshape(1, 1, 4001, 3))
    u8, f01 = G.tensor_to_image(x.numpy())
    want01 = (x * 0.5 + 0.5).clamp(0, 1)
    assert np.array_equal(f01, want01.numpy())
    assert np.array_equal(u8, (want01.numpy() * 255).round().astype("uint8"))


def test_t2img_grid_holds_ties():
    """The fp32 grid of the t2img test holds products exactly on k + 0.5 for even and for odd k (where half-to-even
    and half-away differ, and where they agree), and both clamps."""
    x = G.t2img_fp32_grid()
    assert x.size % 3 == 0
    u8, v = G.tensor_to_image(x.reshape(-1, 3))
    prod = (v * np.float32(255.0)).reshape(-1)
    tie = prod[prod - np.floor(prod) == 0.5]
    even = tie[np.floor(tie) % 2 == 0]
    assert even.size >= 20 and tie.size - even.size >= 20, (tie.size, even.size)
    assert np.array_equal(u8.reshape(-1)[prod - np.floor(prod) == 0.5] % 2, np.zeros(tie.size))    # all went to even
    assert (x < -1).any() and (x > 1).any() and u8.min() == 0 and u8.max() == 255


def test_pack_and_step_outputs():
    rng = np.random.default_rng(1)
    lat = rng.standard_normal((2, 3, 3, 4)).astype(np.float32)
    mask = rng.integers(0, 2, (2, 3, 3)).astype(np.float32)
    masked = rng.standard_normal((2, 3, 3, 4)).astype(np.float32)
    p = G.pack_unet_input(lat, True, 16, mask, masked)
    assert p.shape == (4, 3, 3, 16) and np.array_equal(p[:2], p[2:])
    assert np.array_equal(p[:2, ..., :4], lat) and np.array_equal(p[:2, ..., 4], mask)
    assert np.array_equal(p[:2, ..., 5:9], masked) and not p[..., 9:].any()
    q = G.pack_unet_input(lat, False, 8)
    assert q.shape == (2, 3, 3, 8) and np.array_equal(q[..., :4], lat) and not q[..., 4:].any()
    plan = S.StepPlan(t=1, mode=0, c=(1.0, 0.5, 2.0, 0.0), store_slot=1, save_cur=True)
    slots, cur = [None] * 5, [None]
    eu, ec = rng.standard_normal(lat.shape).astype(np.float32), rng.standard_normal(lat.shape).astype(np.float32)
    o = G.emulate_step(plan, eu, ec, 5.0, lat, slots, cur, cin_pad=8)
    assert np.array_equal(o.eps, slots[1]) and np.array_equal(o.cur, lat) and np.array_equal(cur[0], lat)
    assert np.array_equal(o.unet_in, G.pack_unet_input(o.x, True, 8))
    assert all(v.dtype == np.float32 for v in (o.x, o.eps, o.cur, o.unet_in))
