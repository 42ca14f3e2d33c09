"""CPU tests of the safety-checker restatement `safety_host`, its config and weight handling, the C-ABI exports and the
decisions `RestorationPipeline` takes about when a checker runs (on a stubbed loader: no GPU)."""
import ctypes as C
import json
import logging

import numpy as np
import pytest
import torch
from PIL import Image

from image_restoration_and_enhancement_amd import _lib as L
from image_restoration_and_enhancement_amd import build as B
from image_restoration_and_enhancement_amd import safety_host as H
from image_restoration_and_enhancement_amd import weights as W
from image_restoration_and_enhancement_amd.configs import SafetyConfig
from image_restoration_and_enhancement_amd.inference import RestorationPipeline, SafetyCheckerError
from tests import safetyref as R

REAL = SafetyConfig()          # the SD-1.5 geometry: S = 224


# ------------------------------------------------------------------------------------------- 1. preprocessing
@pytest.mark.parametrize("hw", R.SIZES, ids=lambda s: "x".join(map(str, s)))
def test_uint8_stage_is_pillows(hw):
    """Resize (shortest edge to S, BICUBIC) and centre crop, byte for byte against Pillow driven by hand."""
    img = R.images((1,) + hw)[0]
    h, w = hw
    nh, nw, top, left = H.crop_window(h, w, REAL)
    assert min(nh, nw) == 224 and max(nh, nw) == int(224 * max(h, w) / min(h, w))
    assert (top, left) == ((nh - 224) // 2, (nw - 224) // 2)
    want = np.array(Image.fromarray(img).resize((nw, nh), Image.BICUBIC))[top:top + 224, left:left + 224]
    assert np.array_equal(H.preprocess_u8(img, REAL), want)


@pytest.mark.parametrize("hw", R.SIZES, ids=lambda s: "x".join(map(str, s)))
def test_preprocess_equals_transformers(hw):
    """pixel_values against transformers' CLIPImageProcessor (the PIL backend where torchvision is missing): with the
    processor's operation order — float32(float64(v) * (1 / 255)), then (r - mean) / std in float32 — the result is
    bit-equal on transformers 5.15.  Another version may order the two steps differently (e.g. fused mean / std): that
    is bounded by one float32 ulp of the largest normalised value, (1 - 0.40821073) / 0.26130258 < 4, i.e. 2^-22."""
    tf = pytest.importorskip("transformers")
    proc = tf.CLIPImageProcessor(size=224, crop_size=224, resample=3)
    img = R.images((1,) + hw)[0]
    want = np.asarray(proc(images=Image.fromarray(img), return_tensors="np")["pixel_values"][0])
    got = H.preprocess(img, REAL)[0].numpy()
    assert got.shape == want.shape == (3, 224, 224) and got.dtype == np.float32
    err = float(np.abs(got - want).max())
    print(f"preprocess {hw}: max |d| = {err:.3e}")
    assert err <= 2.0 ** -22
    if tf.__version__ == "5.15.0":
        assert np.array_equal(got, want)


def test_input_table_is_the_processor_order():
    t = H.input_table(REAL).numpy()
    v = np.arange(256, dtype=np.float64)
    r = (v * (1 / 255)).astype(np.float32)
    for c in range(3):
        want = (r - np.float32(REAL.image_mean[c])) / np.float32(REAL.image_std[c])
        assert np.array_equal(t[:, c], want)
    assert t.shape == (256, 3) and t.dtype == np.float32


# ------------------------------------------------------------------------------------------- 2. the tower
# max |d| / max |ref| of vision_pooled against CLIPVisionModel, measured on two CPU hosts (profiles/safety_parity.txt):
# A 2.0e-7 and 2.8e-7, B 1.9e-7 and 2.7e-7 — float32 rounding of the same operations in another association (it moves
# with the BLAS threading).  The bar is ten times the largest measurement.
TOWER_BAR = {"A": 2.8e-6, "B": 2.8e-6}


@pytest.mark.parametrize("name", ["A", "B"])
def test_tower_equals_transformers(name):
    tf = pytest.importorskip("transformers")
    cfg, wd = R.config(name), R.weights(name)
    vc = tf.CLIPVisionConfig(hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                             num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                             patch_size=cfg.patch_size, image_size=cfg.image_size, hidden_act=cfg.hidden_act,
                             layer_norm_eps=cfg.layer_norm_eps, projection_dim=cfg.projection_dim)
    model = tf.CLIPVisionModel(vc).eval()
    keys = list(model.state_dict().keys())
    sd = R.to_transformers_keys(wd, keys)
    assert {k for k in keys if not k.endswith("position_ids")} == set(sd)
    model.load_state_dict(sd, strict=False)
    x = H.preprocess(R.images((2, cfg.image_size + 9, cfg.image_size + 20)), cfg)
    with torch.no_grad():
        want = model(pixel_values=x).pooler_output
    got = H.vision_pooled(x, wd, cfg)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"vision_pooled {name}: max |d| / max |ref| = {err:.3e}")
    assert err < TOWER_BAR[name]
    # image_embeds is the bias-free projection of that
    emb = H.image_embeds(x, wd, cfg)
    assert torch.equal(emb, torch.nn.functional.linear(got, wd["visual_projection.weight"]))
    assert emb.shape == (2, cfg.projection_dim)


# ------------------------------------------------------------------------------------------- 3. the decision
def test_decide_equals_the_diffusers_loop_on_random_rows():
    cs, cc, ts, tc = R.random_rows(1000, seed=11, edge=0.0)
    want = R.diffusers_loop(cs, cc, torch.from_numpy(ts), torch.from_numpy(tc))
    got = H.decide(cs, cc, ts, tc)
    assert np.array_equal(got, want)
    assert 100 < int(want.sum()) < 900            # both outcomes are exercised
    # the rintf form the kernel uses: ((cos - thr) + adj) * 1000 in float32, rint > 0
    m = R.margins(cs, cc, ts, tc)
    concept_hit = (np.rint(m[:, R.N_SPECIAL:] * np.float32(1000.0)) > 0).any(axis=1)
    assert m.dtype == np.float32 and np.array_equal(concept_hit, want)


@pytest.mark.parametrize("name", list(R.DIRECTED))
def test_decide_directed_rows(name):
    emb, special, concepts, ts, tc = R.directed_case(name, 32)
    cs, cc = R.host_cosines(emb, special, concepts, torch.float32)
    assert set(np.unique(cs)) <= {0.0, 1.0} and set(np.unique(cc)) <= {0.0, 1.0}     # exact cosines
    want = R.DIRECTED[name][2]
    assert bool(H.decide(cs, cc, ts, tc)[0]) is want
    assert bool(R.diffusers_loop(cs, cc, torch.from_numpy(ts), torch.from_numpy(tc))[0]) is want


def test_directed_rows_sit_where_they_claim():
    """cos - thr of the deciding concept: -0.005 (lifted by the adjustment or not), 2^-11 and 0.000511."""
    for name, (sx, cx, _) in R.DIRECTED.items():
        _, _, _, ts, tc = R.directed_case(name, 32)
        x = np.float32(1.0) - tc[0]
        assert abs(float(x) - cx) < 2.0 ** -23, name
        if sx is not None:
            assert abs(float(np.float32(1.0) - ts[0]) - sx) < 2.0 ** -23
    assert float(np.float32(1.0) - R.directed_case("below_half", 32)[4][0]) == 2.0 ** -11
    assert float(np.float32(2.0 ** -11) * np.float32(1000.0)) < 0.5


# ------------------------------------------------------------------------------------------- 4. weights and config
def test_check_weights_lists_missing_and_unexpected():
    cfg = R.config("A")
    sd = dict(R.weights("A"))
    sd["vision_model.vision_model.embeddings.position_ids"] = torch.arange(5)[None]      # a buffer: ignored
    assert set(H.check_weights(sd, cfg)) == set(R.weights("A"))
    gone = "vision_model.vision_model.encoder.layers.1.mlp.fc2.bias"
    del sd[gone]
    sd["text_model.final_layer_norm.weight"] = torch.zeros(4)
    with pytest.raises(ValueError) as e:
        H.check_weights(sd, cfg)
    assert gone in str(e.value) and "missing" in str(e.value)
    assert "text_model.final_layer_norm.weight" in str(e.value) and "unexpected" in str(e.value)
    bad = dict(R.weights("A"))
    bad["visual_projection.weight"] = torch.zeros(16, 128)
    with pytest.raises(ValueError, match="visual_projection.weight"):
        H.check_weights(bad, R.config("A"))


def test_param_specs_are_the_real_shapes():
    specs = dict(W.param_specs("safety", SafetyConfig()))
    p = "vision_model.vision_model."
    assert specs[p + "embeddings.patch_embedding.weight"] == (1024, 3, 14, 14)
    assert specs[p + "embeddings.position_embedding.weight"] == (257, 1024)
    assert specs[p + "encoder.layers.23.mlp.fc1.weight"] == (4096, 1024)
    assert specs["visual_projection.weight"] == (768, 1024)
    assert specs["concept_embeds"] == (17, 768) and specs["special_care_embeds_weights"] == (3,)
    assert p + "pre_layrnorm.weight" in specs and p + "encoder.layers.24.mlp.fc1.weight" not in specs
    assert len(specs) == 5 + 24 * 16 + 2 + 5


OLD_FORM = {"crop_size": 224, "do_center_crop": True, "do_normalize": True, "do_resize": True,
            "image_mean": [0.48145466, 0.4578275, 0.40821073], "image_std": [0.26862954, 0.26130258, 0.27577711],
            "resample": 3, "size": 224}
NEW_FORM = dict(OLD_FORM, size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, do_rescale=True,
                rescale_factor=0.00392156862745098)


def test_both_preprocessor_forms_parse():
    for form in (OLD_FORM, NEW_FORM):
        c = SafetyConfig().from_preprocessor(form)
        assert (c.resize_size, c.crop_size, c.rescale_factor) == (224, 224, 1 / 255)
        assert c.image_mean == OLD_FORM["image_mean"] and c.image_std == OLD_FORM["image_std"]
    assert SafetyConfig().from_preprocessor(dict(OLD_FORM, size=256)).resize_size == 256


@pytest.mark.parametrize("change", [dict(resample=2), dict(resample=1), dict(do_resize=False),
                                    dict(do_center_crop=False), dict(do_normalize=False),
                                    dict(size={"height": 224, "width": 224}), dict(crop_size=196),
                                    dict(crop_size={"height": 224, "width": 200}), dict(size=200)])
def test_unsupported_preprocessor_settings_are_refused(change):
    with pytest.raises(ValueError, match="safety checker preprocessor"):
        SafetyConfig().from_preprocessor(dict(OLD_FORM, **change))


def test_config_from_dict_and_load(tmp_path):
    d = tmp_path / "safety_checker"
    d.mkdir()
    cfg = R.config("A")
    (d / "config.json").write_text(json.dumps({"projection_dim": 32, "vision_config": dict(
        R.CONFIGS["A"], hidden_act="quick_gelu", layer_norm_eps=1e-5)}))
    with pytest.raises(FileNotFoundError):
        H.load(d)                                                # no weight file yet
    torch.save(dict(R.weights("A")), str(d / "pytorch_model.bin"))
    (tmp_path / "feature_extractor").mkdir()
    (tmp_path / "feature_extractor" / "preprocessor_config.json").write_text(
        json.dumps(dict(OLD_FORM, size=28, crop_size=28)))
    got_cfg, wd = H.load(d)
    assert got_cfg == cfg
    assert all(torch.equal(wd[k], v) for k, v in R.weights("A").items())
    from safetensors.torch import save_file
    save_file({k: v.half() for k, v in R.weights("A").items()}, str(d / "model.fp16.safetensors"))
    _, wd16 = H.load(d)                                          # preferred over the .bin, read as float32
    assert all(v.dtype == torch.float32 for v in wd16.values())
    assert torch.equal(wd16["concept_embeds"], R.weights("A")["concept_embeds"].half().float())
    with pytest.raises(ValueError, match="activation"):
        SafetyConfig.from_dict({"vision_config": {"hidden_act": "relu"}})


# ------------------------------------------------------------------------------------------- 5. when it runs
def _model_dir(tmp_path, listed, files):
    d = tmp_path / "snapshot"
    (d / "safety_checker").mkdir(parents=True)
    (d / "model_index.json").write_text(json.dumps({
        "_class_name": "StableDiffusionPipeline",
        "safety_checker": ["stable_diffusion", "StableDiffusionSafetyChecker"] if listed else [None, None]}))
    if files:
        (d / "safety_checker" / "config.json").write_text("{}")
        (d / "safety_checker" / "model.safetensors").write_bytes(b"")
    return str(d)


class _Stub:
    def __init__(self, path):
        self.path = path


def _pipe(monkeypatch, engine=None):
    monkeypatch.delenv(H.WEIGHTS_ENV, raising=False)
    p = RestorationPipeline(device="cpu", config=None if engine is None else {"engine": engine})
    loads = []
    monkeypatch.setattr(p, "_load_checker", lambda path: loads.append(path) or _Stub(path))
    return p, loads


def test_auto_follows_model_index(tmp_path, monkeypatch, caplog):
    p, loads = _pipe(monkeypatch)
    assert p.safety_setting == "auto"
    nulls = _model_dir(tmp_path / "a", listed=False, files=True)
    assert p._checker("denoise", nulls) is None                  # the fine-tuned best/ form: [null, null]
    assert p._checker("denoise", str(tmp_path)) is None          # no model_index.json (every test directory so far)
    assert p._checker("denoise", "random") is None
    full = _model_dir(tmp_path / "b", listed=True, files=True)
    c = p._checker("denoise", full)
    assert isinstance(c, _Stub) and c.path == full + "/safety_checker"
    assert p._checker("sr", full) is c and p._checker("colorize", full) is c and loads == [c.path]   # shared
    assert p._checker("inpaint", full) is None
    bare = _model_dir(tmp_path / "c", listed=True, files=False)
    with caplog.at_level(logging.WARNING):
        assert p._checker("denoise", bare) is None
        assert p._checker("sr", bare) is None
    assert caplog.text.count("outputs are not filtered") == 1    # said once


def test_false_a_path_and_the_environment(tmp_path, monkeypatch):
    full = _model_dir(tmp_path, listed=True, files=True)
    p, loads = _pipe(monkeypatch, {"safety_checker": False})
    assert p._checker("denoise", full) is None and loads == []
    p, loads = _pipe(monkeypatch, {"safety_checker": "/some/safety_checker"})
    for task, src in (("denoise", "random"), ("sr", str(tmp_path)), ("colorize", full)):
        assert p._checker(task, src).path == "/some/safety_checker"      # every img2img task, fine-tuned ones too
    assert p._checker("inpaint", full) is None and loads == ["/some/safety_checker"]
    monkeypatch.setenv(H.WEIGHTS_ENV, "/env/safety_checker")
    q = RestorationPipeline(device="cpu")
    assert q.safety_setting == "/env/safety_checker" and q._safety_dir("denoise", "random") == "/env/safety_checker"
    assert q._safety_dir("inpaint", "random") is None
    q = RestorationPipeline(device="cpu", config={"engine": {"safety_checker": False}})      # the key wins
    assert q._safety_dir("denoise", full) is None


def test_a_named_checker_that_cannot_load_is_an_error(tmp_path, monkeypatch):
    monkeypatch.delenv(H.WEIGHTS_ENV, raising=False)
    p = RestorationPipeline(device="cpu", config={"engine": {"safety_checker": str(tmp_path / "none")}})
    with pytest.raises(SafetyCheckerError, match="config.json"):
        p._checker("denoise", "random")
    assert issubclass(SafetyCheckerError, L.IrxError)            # never swallowed by a fallback
    d = tmp_path / "safety_checker"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({"projection_dim": 32, "vision_config": R.CONFIGS["A"]}))
    sd = dict(R.weights("A"))
    del sd["visual_projection.weight"]
    torch.save(sd, str(d / "pytorch_model.bin"))
    p = RestorationPipeline(device="cpu", config={"engine": {"safety_checker": str(d)}})
    with pytest.raises(SafetyCheckerError, match="visual_projection.weight"):
        p._checker("sr", "random")


# ------------------------------------------------------------------------------------------- 6. the C ABI
NEW_SYMBOLS = ("irx_safety_workspace_bytes", "irx_safety_check_u8", "irx_safety_embed_u8", "irx_safety_blank_u8",
               "irx_op_safety_patches", "irx_op_safety_tokens", "irx_op_safety_head")


def test_library_exports_and_bindings():
    lib = C.CDLL(str(B.build()))
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert all(n in L.EXPORTED for n in NEW_SYMBOLS)
    assert L.IRX_MODEL_SAFETY == 6
    names = [f[0] for f in L.ModelConfig._fields_]
    assert names[-5:] == ["image_size", "patch_size", "projection_dim", "n_special", "n_concepts"]
    assert names[-6] == "quick_gelu"                             # appended: nothing before them moved


def test_native_model_refuses_a_bad_config_without_a_gpu():
    """Creation is host-only: the manifest of the real geometry, and the status path for a config it cannot take."""
    from image_restoration_and_enhancement_amd.engine import model_config
    B.build()
    h = C.c_void_p()
    L.call("irx_model_create", L.IRX_MODEL_SAFETY, C.byref(model_config(L.IRX_MODEL_SAFETY, SafetyConfig())),
           L.IRX_F16, C.byref(h))
    n = C.c_int()
    L.call("irx_model_num_params", h, C.byref(n))
    info = L.ParamInfo()
    got = {}
    for i in range(n.value):
        L.call("irx_model_param_info", h, i, C.byref(info))
        got[info.name.decode()] = tuple(int(info.shape[k]) for k in range(info.ndim))
    L.call("irx_model_destroy", h)
    assert got["vision_model.vision_model.embeddings.patch_embedding.weight"] == (1024, 640)     # K 588 -> 640
    assert got["concept_embeds"] == (17, 768) and got["special_care_embeds_weights"] == (3,)
    names = set()
    for k in got:
        names.update(k.split("|"))
    assert names == {k for k, _ in W.param_specs("safety", SafetyConfig())}
    bad = SafetyConfig(image_size=225)
    with pytest.raises(L.IrxError, match="multiple of patch_size"):
        L.call("irx_model_create", L.IRX_MODEL_SAFETY, C.byref(model_config(L.IRX_MODEL_SAFETY, bad)), L.IRX_F16,
               C.byref(h))
