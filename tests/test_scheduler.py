"""CPU tests: scheduler constants and grids (known-answer values), and the host-side step planner
(`schedulers.py`) driven through a float32 emulation of the fused `irx_sched_step` kernel (`tests/glueref.py`;
`tests/test_glue_gpu.py` holds the kernel to it bit for bit) against the oracle's diffusers-0.35.2 restatement
(`oracle/pipeline_ref.py` PNDMRef / DDIMRef).

Known answers are derived by hand from the saved scheduler configs
(`outputs/models/*/best/scheduler/scheduler_config.json`: scaled_linear betas 0.00085..0.012, 1000 train
steps, steps_offset 1, leading spacing) — diffusers itself is absent, so no diffusers-generated vectors.
"""
import numpy as np
import pytest
import torch

from image_restoration_and_enhancement_amd import schedulers as S
from image_restoration_and_enhancement_amd.configs import SchedulerConfig
from oracle import pipeline_ref as PR
from tests.glueref import emulate_step


def test_alphas_cumprod_known_values():
    a = S.alphas_cumprod(SchedulerConfig(kind="pndm"))
    for t, v in ((0, 0.99914998), (1, 0.99829602), (451, 0.34555799), (501, 0.27499884), (999, 0.00466010)):
        assert abs(float(a[t]) - v) < 2e-7, (t, float(a[t]))
    assert torch.equal(a, PR.alphas_cumprod_ref())


@pytest.mark.parametrize("kind,n,strength,expect_first,expect_len", [
    ("pndm", 20, 0.5, 501, 11),      # denoise: PNDM grid [951, 901, 901, 851, ...]; sliced from t_start=10
    ("pndm", 20, 0.8, 801, 17),      # sr default strength
    ("pndm", 30, 0.75, 727, 23),     # colorize
    ("ddim", 30, 0.6, 562, 18),      # inpaint
    ("ddim", 50, 0.5, 481, 25),      # bench: 50 DDIM steps x strength 0.5
])
def test_timestep_grids(kind, n, strength, expect_first, expect_len):
    p = S.make_planner(SchedulerConfig(kind=kind))
    p.set_timesteps(n)
    ts, _ = p.get_timesteps(n, strength)
    ref = PR.PNDMRef() if kind == "pndm" else PR.DDIMRef()
    ref.set_timesteps(n)
    rts, _ = PR.get_timesteps(ref, n, strength)
    assert list(ts) == rts.tolist()
    assert int(ts[0]) == expect_first and len(ts) == expect_len
    assert int(ts[-1]) == 1


def test_pndm_full_grid_duplicate():
    p = S.PNDMPlanner(SchedulerConfig(kind="pndm"))
    p.set_timesteps(20)
    assert p.timesteps[:4].tolist() == [951, 901, 901, 851] and len(p.timesteps) == 21


@pytest.mark.parametrize("kind,n,strength,guidance", [("pndm", 20, 0.5, 5.0), ("pndm", 20, 1.0, 7.5),
                                                      ("pndm", 30, 0.75, 7.5), ("pndm", 20, 0.8, 0.0),
                                                      ("ddim", 30, 0.6, 5.0), ("ddim", 50, 0.5, 5.0)])
def test_planner_matches_oracle_scheduler(kind, n, strength, guidance):
    rng = np.random.default_rng(0)
    p = S.make_planner(SchedulerConfig(kind=kind))
    p.set_timesteps(n)
    ts, _ = p.get_timesteps(n, strength)
    plans = p.plan(ts)
    ref = PR.PNDMRef() if kind == "pndm" else PR.DDIMRef()
    ref.set_timesteps(n)
    x = rng.standard_normal((2, 8, 8, 4)).astype(np.float32)
    xr = torch.from_numpy(x.copy())
    slots = [None] * 5
    cur = [None]
    for plan, t in zip(plans, ts):
        eu = rng.standard_normal(x.shape).astype(np.float32)
        ec = rng.standard_normal(x.shape).astype(np.float32) if guidance > 1 else None
        x = emulate_step(plan, eu, ec, guidance, x, slots, cur).x
        e = torch.from_numpy(eu) + guidance * (torch.from_numpy(ec) - torch.from_numpy(eu)) if ec is not None \
            else torch.from_numpy(eu)
        xr = ref.step(e, int(t), xr)
        np.testing.assert_allclose(x, xr.numpy(), rtol=2e-5, atol=2e-5)


def test_add_noise_coeffs():
    p = S.make_planner(SchedulerConfig(kind="ddim"))
    a, b = p.add_noise_coeffs(501)
    assert abs(a - 0.27499884 ** 0.5) < 1e-6 and abs(b - (1 - 0.27499884) ** 0.5) < 1e-6


def test_strength_zero_slices():
    """strength 0: t_start = N.  PNDM's N+1-entry grid leaves its last step [1]; DDIM leaves nothing."""
    p = S.make_planner(SchedulerConfig(kind="pndm"))
    p.set_timesteps(20)
    ts, n = p.get_timesteps(20, 0.0)
    assert ts.tolist() == [1] and n == 0
    d = S.make_planner(SchedulerConfig(kind="ddim"))
    d.set_timesteps(20)
    ts, n = d.get_timesteps(20, 0.0)
    assert len(ts) == 0 and n == 0
