"""CPU tests of the Real-ESRGAN (SRVGGNetCompact) host restatement `srvgg_host` and of its wiring into
`RestorationPipeline` on `device="cpu"`, with the seeded weights of tests/srvggref.py."""
import logging

import numpy as np
import pytest
import torch
from PIL import Image

from image_restoration_and_enhancement_amd import srvgg_host as H
from image_restoration_and_enhancement_amd.inference import RealESRGANModel, RestorationPipeline
from tests import srvggref as R


@pytest.fixture(scope="module")
def sd():
    return R.seeded_weights(0)


@pytest.fixture(scope="module")
def weights(sd):
    return H.check_weights(sd)


@pytest.fixture(scope="module")
def weight_file(sd, tmp_path_factory):
    path = tmp_path_factory.mktemp("srvgg") / "realesr-seeded.pth"
    torch.save({"params_ema": sd}, str(path))
    return str(path)


# ------------------------------------------------------------------------------------------- weights
def test_weight_specs_are_the_real_shapes():
    specs = dict(H.weight_specs())
    assert len(specs) == 34 * 2 + 33
    assert specs["body.0.weight"] == (64, 3, 3, 3) and specs["body.66.weight"] == (48, 64, 3, 3)
    assert specs["body.34.weight"] == (64, 64, 3, 3) and specs["body.65.weight"] == (64,)
    assert "body.67.weight" not in specs


@pytest.mark.parametrize("nest", ["params_ema", "params", None])
def test_load_weights_round_trip(sd, weights, tmp_path, nest):
    extra = {"params": {"junk": torch.zeros(1)}} if nest == "params_ema" else {}   # params_ema is preferred
    torch.save({nest: sd, **extra} if nest else sd, str(tmp_path / "w.pth"))
    for path in (tmp_path / "w.pth", tmp_path):          # the file, or the directory that holds it
        got = H.load_weights(path)
        assert set(got) == set(weights)
        assert all(torch.equal(got[k], weights[k]) and got[k].dtype == torch.float32 for k in got)


def test_load_weights_refusals(sd, tmp_path):
    with pytest.raises(ValueError) as e:
        H.check_weights(R.rrdb_like())
    assert "conv_first.weight" in str(e.value) and "body.0.rdb1.conv1.weight" in str(e.value)
    assert "missing" in str(e.value) and "body.1.weight" in str(e.value)
    bad = dict(sd)
    bad["body.66.weight"] = torch.zeros(64, 64, 3, 3)
    with pytest.raises(ValueError, match="body.66.weight"):
        H.check_weights(bad)
    with pytest.raises(FileNotFoundError):
        H.load_weights(tmp_path / "none.pth")
    with pytest.raises(FileNotFoundError):
        H.load_weights(tmp_path)                          # a directory without a weight file


# ------------------------------------------------------------------------------------------- the network
def _module(sd):
    layers = []
    for i in range(H.N_CONVS):
        co, ci = H.conv_shape(i)
        layers.append(torch.nn.Conv2d(ci, co, 3, 1, 1))
        if i < H.N_CONVS - 1:
            layers.append(torch.nn.PReLU(num_parameters=64))
    body = torch.nn.Sequential(*layers)
    body.load_state_dict({k[len("body."):]: v for k, v in sd.items()})
    return body.eval(), torch.nn.PixelShuffle(4)


def test_forward_fp32_equals_torch_module(sd, weights):
    body, shuffle = _module(sd)
    x = H.net_input(R.images((2, 9, 13)))
    with torch.no_grad():
        want = shuffle(body(x))
        want += torch.nn.functional.interpolate(x, scale_factor=4, mode="nearest")
    got = H.forward(x, weights, torch.float32)
    assert got.shape == (2, 3, 36, 52) and torch.equal(got, want)


def test_forward_half_rounds_where_the_contract_says(weights):
    x = H.net_input(R.images((1, 5, 7)))
    e = H.forward(x, weights, torch.float64, half=True)
    assert e.dtype == torch.float64 and torch.equal(e.to(torch.float16).double(), e)
    f64 = H.forward(x, weights, torch.float64)
    assert 0 < float((e - f64).abs().max()) < 4e-3


def test_enhance_formula(weights):
    img = R.images((1, 5, 7))[0]
    got = H.enhance(img, weights)
    x = torch.from_numpy((img.astype(np.float32) / 255)[None]).permute(0, 3, 1, 2)
    y = H.forward(x, weights, torch.float32)[0].permute(1, 2, 0).numpy()
    want = np.round(np.clip(y.astype(np.float32), 0, 1) * np.float32(255.0)).astype(np.uint8)
    assert isinstance(got, np.ndarray) and got.shape == (20, 28, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want)
    assert np.array_equal(H.input_table().numpy(), np.arange(256, dtype=np.float32) / 255)
    batch = H.enhance(torch.from_numpy(np.stack([img, img[::-1].copy()])), weights)
    assert np.array_equal(batch[0].numpy(), got) and batch.shape == (2, 20, 28, 3)


# ------------------------------------------------------------------------------------------- drop-in on the CPU
def _config(backend, path=None):
    sr = {"fine_tuned_dir": "missing", "pretrained_id": "unused", "default_backend": backend}
    if path is not None:
        sr["realesrgan_weights"] = path
    return {"sr": sr}


def test_pipeline_realesrgan_on_cpu(weights, weight_file):
    img = Image.fromarray(R.images((1, 6, 9))[0])
    want = H.enhance(np.array(img), weights)
    pipe = RestorationPipeline(device="cpu", config=_config("realesrgan", weight_file))
    got = pipe.super_resolve(img)
    assert isinstance(pipe.models["sr"], RealESRGANModel) and hasattr(pipe.models["sr"], "enhance")
    assert got.size == (36, 24) and np.array_equal(np.array(got), want)
    half = pipe.super_resolve(img, scale=2)
    assert half.size == (18, 12)
    assert np.array_equal(np.array(half), np.array(Image.fromarray(want).resize((18, 12), Image.LANCZOS)))
    assert np.array_equal(np.array(pipe.process(img, ["sr"])["final"]), want)
    # "auto" with the same weights lands on the model after the failed SD load
    auto = RestorationPipeline(device="cpu", config=_config("auto", weight_file))
    assert np.array_equal(np.array(auto.super_resolve(img)), want)
    assert isinstance(auto.models["sr"], RealESRGANModel)


def test_restore_batch_on_cpu(weight_file):
    pipe = RestorationPipeline(device="cpu", config=_config("realesrgan", weight_file))
    ims = [Image.fromarray(R.images((1, 5, 8), seed=s)[0]) for s in (1, 2)]
    ims.insert(1, Image.fromarray(R.images((1, 4, 9), seed=3)[0]))
    for im, r in zip(ims, pipe.restore_batch("sr", ims)):
        assert np.array_equal(np.array(r), np.array(pipe.super_resolve(im)))


def test_corrupt_file(tmp_path):
    bad = tmp_path / "bad.pth"
    torch.save(R.rrdb_like(), str(bad))
    with pytest.raises(RuntimeError, match="Real-ESRGAN loading failed"):
        RestorationPipeline(device="cpu", config=_config("realesrgan", str(bad))).load_sr_model()
    (tmp_path / "garbage.pth").write_bytes(b"not a checkpoint")
    with pytest.raises(RuntimeError, match="Real-ESRGAN loading failed"):
        RestorationPipeline(device="cpu", config=_config("realesrgan", str(tmp_path / "garbage.pth"))).load_sr_model()
    auto = RestorationPipeline(device="cpu", config=_config("auto", str(bad)))
    auto.load_sr_model()
    assert auto.models["sr"] == "lanczos"


def test_nothing_configured_is_as_before(monkeypatch):
    monkeypatch.delenv(H.WEIGHTS_ENV, raising=False)
    with pytest.raises(ImportError, match="Real-ESRGAN is not available"):
        RestorationPipeline(device="cpu", config=_config("realesrgan")).load_sr_model()
    auto = RestorationPipeline(device="cpu", config=_config("auto"))
    auto.load_sr_model()
    assert auto.models["sr"] == "lanczos"
    img = Image.fromarray(R.images((1, 6, 9))[0])
    assert np.array_equal(np.array(auto.super_resolve(img)), np.array(img.resize((36, 24), Image.LANCZOS)))


def test_weights_from_the_environment(weights, weight_file, monkeypatch):
    monkeypatch.setenv(H.WEIGHTS_ENV, weight_file)
    pipe = RestorationPipeline(device="cpu", config=_config("realesrgan"))
    img = Image.fromarray(R.images((1, 6, 9))[0])
    assert np.array_equal(np.array(pipe.super_resolve(img)), H.enhance(np.array(img), weights))


def test_enhance_failure_takes_lanczos(weight_file, caplog):
    pipe = RestorationPipeline(device="cpu", config=_config("realesrgan", weight_file))
    pipe.load_sr_model()
    pipe.models["sr"].weights = {}                         # enhance now raises KeyError
    img = Image.fromarray(R.images((1, 6, 9))[0])
    with caplog.at_level(logging.WARNING):
        out = pipe.super_resolve(img)
    assert np.array_equal(np.array(out), np.array(img.resize((36, 24), Image.LANCZOS)))
    assert "Real-ESRGAN upscaling failed" in caplog.text
