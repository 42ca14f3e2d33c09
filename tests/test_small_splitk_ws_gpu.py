"""K-split partials of the small-M GEMMs (the time embedding's linear_2, gemm_plan.cpp small_splits) live in the caller's
workspace: gemm_workspace_bytes reports them and the models carve them from their arena, so a captured denoising loop
holds no pointer into the library's grow-on-demand scratch, which a later call with more rows frees and reallocates."""
import numpy as np
import pytest
import torch

from oracle import pipeline_ref as PR
from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd.configs import PipelineConfig
from image_restoration_and_enhancement_amd.pipelines import SDEngine
from tests import models_common as MC


@pytest.mark.parametrize("dtype", [L.IRX_BF16, L.IRX_F16])
@pytest.mark.parametrize("rows", [2, 16, 25, 50])
def test_workspace_bytes_cover_time_embedding_splits(dtype, rows):
    """time_embedding.linear_2 ([rows] x 1280 x 1280, SiLU): 20 column tiles -> 4 K splits of fp32 partials.
    (A host-side shape query: no GPU needed.)"""
    got = L.call("irx_op_gemm_workspace_bytes", dtype, rows, 1280, 1280, 1, 0, rows)
    assert got == 4 * rows * 1280 * 4
    # short K (linear_1) and the 315-tile time_emb_proj GEMM take no splits
    assert L.call("irx_op_gemm_workspace_bytes", dtype, rows, 1280, 320, 1, 0, rows) == 0
    assert L.call("irx_op_gemm_workspace_bytes", dtype, rows, 20160, 1280, 0, 1, rows) == 0


@pytest.mark.gpu
def test_graph_replay_survives_larger_eager_call(device):
    """Capture a small-batch loop, run a larger-batch eager loop (more rows through every small-M GEMM), replay the
    old graph: the same bits as its first replay."""
    prompt, strength, steps, guidance = PR.TASKS["denoise"]
    pc, sd = MC.state_dicts("denoise")
    cfg = PipelineConfig.default("denoise")
    cfg.scheduler.kind = "ddim"
    eng = SDEngine(cfg, "bf16", device, state_dicts=sd)
    small = torch.from_numpy(MC.smooth_image(64, 64, seed=60)[None]).to(device)
    big = torch.from_numpy(np.stack([MC.smooth_image(64, 64, seed=61 + i) for i in range(5)])).to(device)

    def run(x):
        return eng.img2img(x, prompt, strength, 50, guidance, seed=42, n_evals=2)
    run(small)                      # eager + capture
    first = run(small)              # replay
    eng.use_graphs = False
    run(big)                        # eager, 10 rows per evaluation instead of 2
    eng.use_graphs = True
    again = run(small)              # replay of the graph captured before
    assert len(eng._graphs) == 1
    assert torch.equal(again.latents, first.latents)
    assert torch.equal(again.images_u8, first.images_u8)
