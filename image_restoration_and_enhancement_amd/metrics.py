"""Evaluation metrics — numpy/scipy/PIL restatement of the reference's `src/metrics.py`.

The reference imports cv2, scikit-image and torchvision (`src/metrics.py:11-22`) and exits when any
is missing; none of them is installed on the GPU image, so `scripts/evaluate_model.py --no-lpips
--no-fid` could not run there.  This module keeps the same surface (`load_image`,
`MetricsCalculator.calculate_{psnr,ssim,delta_e,all}`, `evaluate_task`, `print_results`) with the
arithmetic restated:

* PSNR  = skimage `peak_signal_noise_ratio(gt, pred, data_range=255)` (`src/metrics.py:82-87`)
* SSIM  = skimage `structural_similarity(gt, pred, data_range=255, channel_axis=2)` defaults:
  7x7 uniform window (scipy `uniform_filter`, reflect borders), sample covariance (NP/(NP-1)),
  K1 = 0.01, K2 = 0.03, mean over the map cropped by 3 px, mean over channels (`:89-95`)
* dE76  = mean Euclidean distance of skimage `rgb2lab` (D65, 2 deg) of pred/255 and gt/255 (`:115-148`)
* shape mismatch: pred resized to gt with cv2 `INTER_LINEAR` semantics (half-pixel centres,
  11-bit fixed-point weights, round-to-nearest) (`:84-85`)
* `load_image`: `cv2.imread` + BGR->RGB == PIL decode to RGB (`:40-46`)

PSNR / SSIM / rgb2lab are pinned against scikit-image 0.18.3 outputs committed under
`tests/golden/metrics.json` (tests/test_metrics.py).  The INTER_LINEAR resize and JPEG decode are
restatements without an oracle in this image (cv2 is absent): parity unpinned.

FID (`src/metrics.py:150-223`) is computed when the user points at torchvision's InceptionV3 checkpoint —
`fid_weights=` or the environment variable `IRX_FID_WEIGHTS` (`fid_host.load_weights`); the code is `fid_host`
(plain torch) on the host and `fid_gpu` (csrc/fid_model.cpp, csrc/fid.hip) with `device="cuda"`; the distance itself
is the reference's numpy / scipy arithmetic (`fid_host.frechet_distance`).  With nothing configured the metric is off
as before: `use_fid` is False, `calculate_fid` returns None, `evaluate_task` reports no `fid` entry, and the module
constant `FID_AVAILABLE` (torchvision itself) stays False.  A path that is set but cannot be read is an error.

LPIPS(alex) (`src/metrics.py:97-111`) is computed when the user points at the two weight files it needs —
`lpips_weights=` or the environment variable `IRX_LPIPS_WEIGHTS` (a directory or a file, `lpips_host.load_weights`);
the code is `lpips_host` (plain torch) on the host and `lpips_gpu` (csrc/lpips.hip) with `device="cuda"`.  With
nothing configured the metric is off as before: `use_lpips` is False, `calculate_lpips` returns None, and the module
constant `LPIPS_AVAILABLE` (the `lpips` package itself) stays False.  A path that is set but cannot be read is an error.

With `device="cuda"` the calculator and `evaluate_task` score on the GPU (`metrics_gpu`, csrc/metrics.hip): PSNR
bit-equal to the functions below, SSIM and dE76 to 1e-9.  The module-level functions and
`device="cpu"` are the numpy code and the oracle of that path.
"""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np
from PIL import Image
from scipy.ndimage import uniform_filter

LPIPS_AVAILABLE = False
FID_AVAILABLE = False
LPIPS_WEIGHTS_ENV = "IRX_LPIPS_WEIGHTS"
FID_WEIGHTS_ENV = "IRX_FID_WEIGHTS"

# skimage.color: sRGB (D65) -> XYZ and the D65 / 2-degree white point
_XYZ_FROM_RGB = np.array([[0.412453, 0.357580, 0.180423],
                          [0.212671, 0.715160, 0.072169],
                          [0.019334, 0.119193, 0.950227]])
_WHITE_D65 = np.array([0.95047, 1.0, 1.08883])


def load_image(path: Path, device=None):
    """Load image as RGB uint8 HWC (reference `src/metrics.py:40-46`).  With a `cuda*` device and a .jpg / .jpeg name
    the file is decoded on the GPU (`jpeg_gpu.open`, csrc/jpeg_decode.hip; the same pixels) and the result is a uint8
    device tensor; otherwise, and where the native path is not available, a numpy array, as ever."""
    if device is not None and str(device).startswith("cuda") and Path(path).suffix.lower() in (".jpg", ".jpeg"):
        try:
            from . import _lib, jpeg_gpu
            try:
                return jpeg_gpu.open(Path(path), "RGB", device)
            except _lib.IrxError:       # no library, or an argument the op refuses (a scan above 128 MiB): PIL below
                pass
        except ImportError:             # no torch
            pass
        except (OSError, ValueError):
            raise ValueError(f"Could not load image: {path}")
    try:
        with Image.open(str(path)) as im:
            return np.array(im.convert("RGB"))
    except (OSError, ValueError):
        raise ValueError(f"Could not load image: {path}")


def linear_axis(n_out: int, n_in: int):
    """One axis of cv2's INTER_LINEAR for uint8: (i0, i1, w0, w1) per output index, the two source indices and
    their 11-bit weights (w0 + w1 = 2048).  Shared by `resize_linear` and the GPU tables (`metrics_gpu`)."""
    scale = n_in / n_out
    f = (np.arange(n_out) + 0.5) * scale - 0.5
    i0 = np.floor(f).astype(np.int64)
    f = f - i0
    lo = i0 < 0
    f[lo], i0[lo] = 0.0, 0
    hi = i0 >= n_in - 1
    f[hi], i0[hi] = 0.0, n_in - 1
    w1 = np.rint(f * 2048).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_in - 1), 2048 - w1, w1


def resize_linear(img: np.ndarray, width: int, height: int) -> np.ndarray:
    """cv2.resize(img, (width, height)) with INTER_LINEAR for uint8 images."""
    H, W = img.shape[:2]
    if (H, W) == (height, width):
        return img.copy()
    y0, y1, wy0, wy1 = linear_axis(height, H)
    x0, x1, wx0, wx1 = linear_axis(width, W)
    a = img.astype(np.int64)
    if a.ndim == 2:
        a = a[..., None]
    rows = a[:, x0] * wx0[None, :, None] + a[:, x1] * wx1[None, :, None]        # [H, width, C]
    out = rows[y0] * wy0[:, None, None] + rows[y1] * wy1[:, None, None]
    out = (out + (1 << 21)) >> 22
    out = np.clip(out, 0, 255).astype(np.uint8)
    return out[..., 0] if img.ndim == 2 else out


def psnr(gt: np.ndarray, pred: np.ndarray, data_range: float = 255.0) -> float:
    err = np.mean((gt.astype(np.float64) - pred.astype(np.float64)) ** 2)
    with np.errstate(divide="ignore"):
        return float(10 * np.log10((data_range ** 2) / err))


def _ssim_2d(X: np.ndarray, Y: np.ndarray, data_range: float, win: int = 7, K1: float = 0.01,
             K2: float = 0.03) -> float:
    X = X.astype(np.float64)
    Y = Y.astype(np.float64)
    NP = win * win
    cov_norm = NP / (NP - 1)
    ux = uniform_filter(X, size=win)
    uy = uniform_filter(Y, size=win)
    uxx = uniform_filter(X * X, size=win)
    uyy = uniform_filter(Y * Y, size=win)
    uxy = uniform_filter(X * Y, size=win)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    C1 = (K1 * data_range) ** 2
    C2 = (K2 * data_range) ** 2
    A1, A2 = 2 * ux * uy + C1, 2 * vxy + C2
    B1, B2 = ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    pad = (win - 1) // 2
    return float(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean())


def ssim(gt: np.ndarray, pred: np.ndarray, data_range: float = 255.0) -> float:
    if gt.shape != pred.shape:
        raise ValueError("Input images must have the same dimensions.")
    if gt.ndim == 2:
        return _ssim_2d(gt, pred, data_range)
    return float(np.mean([_ssim_2d(gt[..., c], pred[..., c], data_range) for c in range(gt.shape[2])]))


def srgb_linear(rgb: np.ndarray) -> np.ndarray:
    """The sRGB linearisation in front of skimage's rgb2xyz, in the dtype of `rgb` (float32 for the dE path)."""
    arr = np.array(rgb, copy=True)
    mask = arr > 0.04045
    arr[mask] = np.power((arr[mask] + 0.055) / 1.055, 2.4)
    arr[~mask] /= 12.92
    return arr


def rgb2lab(rgb: np.ndarray) -> np.ndarray:
    """skimage.color.rgb2lab for float RGB in [0, 1] (D65, 2-degree observer)."""
    return lab_from_linear(srgb_linear(rgb))


def lab_from_linear(arr: np.ndarray) -> np.ndarray:
    """rgb2lab after the linearisation (fp64 from here on): XYZ, white point, cbrt / linear branch, Lab."""
    xyz = arr @ _XYZ_FROM_RGB.T
    xyz = xyz / _WHITE_D65
    mask = xyz > 0.008856
    xyz[mask] = np.cbrt(xyz[mask])
    xyz[~mask] = 7.787 * xyz[~mask] + 16.0 / 116.0
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    return np.stack([116.0 * y - 16.0, 500.0 * (x - y), 200.0 * (y - z)], axis=-1)


def _to_host(img) -> np.ndarray:
    """A numpy image from a numpy image or a (device) tensor."""
    return img if isinstance(img, np.ndarray) else img.detach().cpu().numpy()


def resolve_lpips_weights(lpips_weights=None):
    """The LPIPS(alex) weights as a checked dict, or None when nothing is configured: `lpips_weights` (a dict of
    tensors, or a directory / file for `lpips_host.load_weights`), else the path in `IRX_LPIPS_WEIGHTS`.  A source
    that is given but cannot be read raises."""
    src = lpips_weights if lpips_weights is not None else (os.environ.get(LPIPS_WEIGHTS_ENV) or None)
    if src is None:
        return None
    from . import lpips_host
    return lpips_host.check_weights(src) if isinstance(src, dict) else lpips_host.load_weights(src)


def resolve_fid_weights(fid_weights=None):
    """The InceptionV3 weights as a checked dict, or None when nothing is configured: `fid_weights` (a dict of
    tensors, or a directory / file for `fid_host.load_weights`), else the path in `IRX_FID_WEIGHTS`.  A source that
    is given but cannot be read raises."""
    src = fid_weights if fid_weights is not None else (os.environ.get(FID_WEIGHTS_ENV) or None)
    if src is None:
        return None
    from . import fid_host
    return fid_host.check_weights(src) if isinstance(src, dict) else fid_host.load_weights(src)


class _FidCollector:
    """The Inception features of a growing set of (pred, gt) pairs without keeping the images: on the GPU through
    `fid_gpu.FeatureQueue` (one queue per side, enqueued, nothing waits), else `fid_host` in float32 right away."""

    def __init__(self, calc: "MetricsCalculator"):
        self.calc = calc
        self.net = calc._fid_network()
        self.host = ([], [])
        self.queues = None
        if self.net is not None:
            from . import fid_gpu
            self.queues = (fid_gpu.FeatureQueue(self.net), fid_gpu.FeatureQueue(self.net))

    def add(self, pred, gt) -> None:
        """One pair; `pred` goes to gt's size first (cv2.resize in the reference, `src/metrics.py:190-191`)."""
        calc = self.calc
        if self.queues is not None and all(len(x.shape) == 3 and x.shape[2] == 3 for x in (pred, gt)):
            G = calc._gpu_module()
            p, g = G.to_device(pred, calc.device), G.to_device(gt, calc.device)
            if tuple(p.shape[:2]) != tuple(g.shape[:2]):
                p = G.resize_linear_u8(p, g.shape[1], g.shape[0])
            self.queues[0].add(p)
            self.queues[1].add(g)
            return
        from . import fid_host
        pred, gt = _to_host(pred), _to_host(gt)
        if pred.shape[:2] != gt.shape[:2]:
            pred = resize_linear(pred, gt.shape[1], gt.shape[0])
        for side, im in zip(self.host, (pred, gt)):
            side.append(fid_host.features_u8([im], calc._fid_w))

    def device_features(self):
        """Device float32 [2, n, 2048] of the pairs that went through the GPU (pred set, gt set), or None."""
        if self.queues is None or len(self.queues[0]) == 0:
            return None
        return self.calc._gpu.torch.stack([q.finish() for q in self.queues])

    def score(self, dev_feats=None) -> float:
        """The Fréchet distance of everything collected; `dev_feats` is `device_features()` already on the host."""
        import torch
        sets = []
        for k in range(2):
            parts = list(self.host[k])
            if dev_feats is not None:
                parts.append(torch.as_tensor(np.asarray(dev_feats[k], dtype=np.float32)))
            sets.append(torch.cat(parts, 0).numpy())
        from . import fid_host
        return fid_host.frechet_distance(sets[0], sets[1])


class MetricsCalculator:
    """Per-image metrics (reference `src/metrics.py:57-209`).  LPIPS(alex) and FID: on when their weights are
    configured (`lpips_weights` / `IRX_LPIPS_WEIGHTS`, `fid_weights` / `IRX_FID_WEIGHTS`), see the module docstring.

    `device="cpu"` (the default) is the numpy code above.  A `cuda*` string or torch.device scores on the GPU
    (`metrics_gpu`, csrc/metrics.hip) when one is visible, `libirx.so` loads and the pair's shape is inside the
    kernel's range (H, W >= 7, 1 or 3 channels); any other pair takes the numpy code.  Every method accepts numpy
    images or uint8 device tensors ([H, W] or [H, W, C]), so `restore_batch` outputs are scored without a download.

    `decode="gpu"` makes `load` decode .jpg / .jpeg files on that GPU (`load_image(path, device)`), so the pixels of a
    pair never visit the host; `decode="pil"` (the default), a CPU device and every other file type load with PIL."""

    def __init__(self, use_lpips: bool = True, use_fid: bool = True, device: str = "cpu", lpips_weights=None,
                 fid_weights=None, decode: str = "pil"):
        if decode not in ("pil", "gpu"):
            raise ValueError("decode must be 'pil' or 'gpu'")
        self.decode = decode
        self._lpips_w = resolve_lpips_weights(lpips_weights) if use_lpips else None
        self.use_lpips = self._lpips_w is not None
        self._fid_w = resolve_fid_weights(fid_weights) if use_fid else None
        self.use_fid = self._fid_w is not None
        self._fid_net = None    # fid_gpu.InceptionFeatures, made at the first GPU feature call
        self.device = device
        self._gpu = False       # metrics_gpu, None (host), or False: not decided yet
        self._lpips_net = None  # lpips_gpu.LpipsAlex, made at the first GPU score

    def _gpu_module(self):
        """`metrics_gpu` when `device` names a GPU, one is visible and the native library loads; else None."""
        if self._gpu is False:
            self._gpu = None
            if str(self.device).startswith("cuda"):
                try:
                    import torch
                    if torch.cuda.is_available():
                        from . import _lib, metrics_gpu
                        _lib.load()
                        self._gpu = metrics_gpu
                except Exception:   # no torch, no library: the host code serves
                    self._gpu = None
        return self._gpu

    def load(self, path):
        """`load_image(path)`, on the device where `decode="gpu"` and the GPU path is up."""
        if self.decode == "gpu" and self._gpu_module() is not None:
            return load_image(path, self.device)
        return load_image(path)

    def _device_pair(self, pred, gt, channels=(1, 3)):
        """(pred, gt) as uint8 device tensors of gt's shape (pred resized on the GPU if its size differs), or None
        when this pair takes the host code.  Two numpy images of one shape go up in one copy."""
        G = self._gpu_module()
        ps, gs = tuple(pred.shape), tuple(gt.shape)
        if G is None or len(ps) != len(gs) or len(gs) not in (2, 3) or ps[2:] != gs[2:] or not G.supported(gs):
            return None
        if (gs[2] if len(gs) == 3 else 1) not in channels or min(ps[:2]) < 1:
            return None
        if any(str(x.dtype).rsplit(".", 1)[-1] != "uint8" for x in (pred, gt)):     # numpy or torch dtype
            return None
        if ps == gs and isinstance(pred, np.ndarray) and isinstance(gt, np.ndarray):
            both = G.to_device(np.stack([pred, gt]), self.device)
            return both[0], both[1]
        p, g = G.to_device(pred, self.device), G.to_device(gt, self.device)
        if ps != gs:
            p = G.resize_linear_u8(p, gs[1], gs[0])
        return p, g

    def _device_stats(self, pred, gt, pair=None):
        """(device float64 [2] = (squared error, SSIM), values per image) without waiting for the device, or None
        when this pair takes the host code.  The squared error is an integer below 2^53: exact as a double."""
        pair = self._device_pair(pred, gt) if pair is None else pair
        if pair is None:
            return None
        sse, ssim_, _ = self._gpu.pair_stats(pair[0], pair[1])
        return self._gpu.torch.cat([sse.to(ssim_.dtype), ssim_]), pair[1].numel()

    def _lpips_pair(self, pair):
        """Device float64 [1]: LPIPS of a `_device_pair` result, enqueued without waiting; None when the pair is
        outside the GPU model's range (not RGB, a side below 31) and the host code decides."""
        if pair is None:
            return None
        from . import lpips_gpu
        if not lpips_gpu.supported(pair[1].shape):
            return None
        if self._lpips_net is None:
            self._lpips_net = lpips_gpu.LpipsAlex(self._lpips_w, self.device)
        return self._lpips_net.score(pair[0], pair[1])

    def _lpips_host(self, pred, gt) -> float:
        from . import lpips_host
        pred, gt = _to_host(pred), _to_host(gt)
        return float(lpips_host.lpips_alex(self._match(pred, gt), gt, self._lpips_w)[0][0])

    @staticmethod
    def _match(pred: np.ndarray, gt: np.ndarray) -> np.ndarray:
        return pred if pred.shape == gt.shape else resize_linear(pred, gt.shape[1], gt.shape[0])

    def calculate_psnr(self, pred: np.ndarray, gt: np.ndarray) -> float:
        pair = self._device_pair(pred, gt)
        if pair is not None:
            return self._gpu.psnr_from_sse(self._gpu.pair_stats(*pair)[0][0].item(), pair[1].numel())
        pred, gt = _to_host(pred), _to_host(gt)
        return psnr(gt, self._match(pred, gt), data_range=255.0)

    def calculate_ssim(self, pred: np.ndarray, gt: np.ndarray) -> float:
        pair = self._device_pair(pred, gt)
        if pair is not None:
            return float(self._gpu.pair_stats(*pair)[1][0].item())
        pred, gt = _to_host(pred), _to_host(gt)
        return ssim(gt, self._match(pred, gt), data_range=255.0)

    def calculate_lpips(self, pred: np.ndarray, gt: np.ndarray):
        """LPIPS(alex) of one pair (reference `src/metrics.py:97-111`), or None when no weights are configured."""
        if not self.use_lpips:
            return None
        dev = self._lpips_pair(self._device_pair(pred, gt, channels=(3,)))
        return float(dev[0].item()) if dev is not None else self._lpips_host(pred, gt)

    def calculate_delta_e(self, pred: np.ndarray, gt: np.ndarray, use_delta_e2000: bool = False) -> float:
        pair = self._device_pair(pred, gt, channels=(3,))
        if pair is not None:
            return float(self._gpu.pair_stats(*pair, delta_e=True)[2][0].item())
        pred, gt = _to_host(pred), _to_host(gt)
        pred = self._match(pred, gt)
        pl = rgb2lab(pred.astype(np.float32) / 255.0)
        gl = rgb2lab(gt.astype(np.float32) / 255.0)
        return float(np.mean(np.sqrt(np.sum((pl - gl) ** 2, axis=2))))

    def _fid_network(self):
        """`fid_gpu.InceptionFeatures` when `device` names a visible GPU and the native library loads; else None."""
        if self._gpu_module() is None:
            return None
        if self._fid_net is None:
            from . import fid_gpu
            self._fid_net = fid_gpu.InceptionFeatures(self._fid_w, self.device)
        return self._fid_net

    def calculate_fid(self, pred_images, gt_images):
        """FID of two image sets (reference `src/metrics.py:164-223`), or None when no weights are configured.
        Images are uint8 RGB numpy arrays or device tensors of any sizes; features come from the GPU with a `cuda*`
        device (one download of the two [N, 2048] sets), else from `fid_host` in float32."""
        if not self.use_fid:
            return None
        if len(pred_images) != len(gt_images):
            print(f"Warning: FID requires equal number of images. Got {len(pred_images)} pred vs {len(gt_images)} gt")
            return None
        print("  Extracting Inception features for FID...")
        col = _FidCollector(self)
        for pred, gt in zip(pred_images, gt_images):
            col.add(pred, gt)
        dev = col.device_features()
        return col.score(None if dev is None else dev.cpu().numpy())

    def calculate_all(self, pred: np.ndarray, gt: np.ndarray) -> dict:
        pair = self._device_pair(pred, gt)      # one upload, the resize if the shapes differ
        if pair is not None:                    # one pair_stats call, LPIPS behind it, one download
            dev = self._device_stats(pred, gt, pair)
            lp = self._lpips_pair(pair) if self.use_lpips else None
            v = (dev[0] if lp is None else self._gpu.torch.cat([dev[0], lp])).cpu().numpy()
            out = {"psnr": self._gpu.psnr_from_sse(int(v[0]), dev[1]), "ssim": float(v[1])}
            if self.use_lpips:
                out["lpips"] = float(v[2]) if lp is not None else self._lpips_host(pred, gt)
            return out
        out = {"psnr": self.calculate_psnr(pred, gt), "ssim": self.calculate_ssim(pred, gt)}
        if self.use_lpips:
            out["lpips"] = self.calculate_lpips(pred, gt)
        return out


_EXTS = {".jpg", ".jpeg", ".png"}


def evaluate_task(pred_dir: Path, gt_dir: Path, task_name: str = "denoise", use_lpips: bool = True,
                  use_fid: bool = True, device: str = "cpu", lpips_weights=None, fid_weights=None,
                  decode: str = "pil") -> dict:
    """Match predictions to ground truth by file name (any of .jpg/.jpeg/.png) and aggregate
    mean/std/min/max/median per metric (reference `src/metrics.py:238-348`).  With a `cuda*` device the pairs are
    scored on the GPU as they are loaded and read back together, one synchronisation per task.  LPIPS is reported
    when weights are configured (`lpips_weights` or `IRX_LPIPS_WEIGHTS`); a pair it refuses (a side below 31 px) is
    skipped whole, as the reference skips a pair whose `calculate_all` raises.  FID is reported (`fid`, one value)
    when weights are configured (`fid_weights` or `IRX_FID_WEIGHTS`): each scored pair's Inception features are
    taken as the loop runs — the reference keeps every image in a list instead — and read back with the rest.
    `decode="gpu"` (with a `cuda*` device) decodes the .jpg / .jpeg files of the pairs on the GPU as well
    (`jpeg_gpu`), so their pixels never visit the host; the result is the same to the last bit."""
    pred_dir, gt_dir = Path(pred_dir), Path(gt_dir)
    calc = MetricsCalculator(use_lpips=use_lpips, use_fid=use_fid, device=device, lpips_weights=lpips_weights,
                             fid_weights=fid_weights, decode=decode)
    pred_files = sorted(f for f in pred_dir.iterdir() if f.suffix.lower() in _EXTS)
    gt_names = {f.name for f in gt_dir.iterdir() if f.suffix.lower() in _EXTS}
    if len(pred_files) != len(gt_names):
        print(f"Warning: Mismatch - {len(pred_files)} predictions vs {len(gt_names)} ground truth")
    pairs = []
    for pf in pred_files:
        gf = gt_dir / pf.name
        if not gf.exists():
            for ext in (".jpg", ".jpeg", ".png"):
                alt = gt_dir / (pf.stem + ext)
                if alt.exists():
                    gf = alt
                    break
        if gf.exists():
            pairs.append((pf, gf))
    if not pairs:
        raise ValueError(f"No matching files found between {pred_dir} and {gt_dir}")
    all_metrics = {"psnr": [], "ssim": []}
    if calc.use_lpips:
        all_metrics["lpips"] = []
    print(f"Evaluating {task_name}: {len(pairs)} image pairs...")
    # GPU path: (slot in the lists, device (squared error, SSIM[, LPIPS]), values per image, LPIPS on the device)
    pending = []
    fid, fid_error = None, None
    if calc.use_fid:
        try:
            fid = _FidCollector(calc)
        except Exception as e:
            fid_error = e
    for i, (pp, gp) in enumerate(pairs):
        try:
            pred, gt = calc.load(pp), calc.load(gp)
            pair = calc._device_pair(pred, gt)
            if pair is not None:                # enqueued; read back after the loop, all pairs in one download
                # LPIPS first: a pair it refuses raises here, before any slot of the pair exists
                lp = calc._lpips_pair(pair) if calc.use_lpips else None
                lp_host = calc._lpips_host(pred, gt) if calc.use_lpips and lp is None else None
                stats, n = calc._device_stats(pred, gt, pair)
                if lp is not None:
                    stats = calc._gpu.torch.cat([stats, lp])
                pending.append((len(all_metrics["psnr"]), stats, n, lp is not None))
                all_metrics["psnr"].append(None)
                all_metrics["ssim"].append(None)
                if calc.use_lpips:
                    all_metrics["lpips"].append(lp_host)
            else:
                for k, v in calc.calculate_all(pred, gt).items():
                    if v is not None:
                        all_metrics[k].append(v)
            if fid is not None and fid_error is None:       # after the pair's own metrics: a skipped pair is not in
                try:                                        # the tensors already on the device, where there are any
                    fid.add(*(pair if pair is not None else (pred, gt)))
                except Exception as e:
                    fid_error = e
            if (i + 1) % 10 == 0:
                print(f"  Processed {i + 1}/{len(pairs)}")
        except Exception as e:  # the reference skips unreadable pairs
            print(f"Error processing {pp.name}: {e}")
    fid_dev = None
    if fid is not None and fid_error is None:
        try:
            fid_dev = fid.device_features()
        except Exception as e:
            fid_error = e
    fid_host_feats = None
    if fid_dev is not None and not pending:
        fid_host_feats = fid_dev.cpu().numpy()
    if pending:
        G = calc._gpu_module()
        parts = [t for _, t, _, _ in pending]
        if fid_dev is not None:             # float32 -> float64 is exact: the features ride in the same download
            parts.append(fid_dev.reshape(-1).to(parts[0].dtype))
        vals = G.torch.cat(parts).cpu().numpy()                            # the task's one synchronisation
        if fid_dev is not None:
            fid_host_feats = vals[-fid_dev.numel():].reshape(tuple(fid_dev.shape))
        at = 0
        for slot, t, n, has_lp in pending:
            v = vals[at:at + t.numel()]
            at += t.numel()
            all_metrics["psnr"][slot] = G.psnr_from_sse(int(v[0]), n)
            all_metrics["ssim"][slot] = float(v[1])
            if has_lp:
                all_metrics["lpips"][slot] = float(v[2])
    if calc.use_fid:
        print("\n  Calculating FID (dataset-level metric)...")
        try:
            if fid_error is not None:
                raise fid_error
            all_metrics["fid"] = [fid.score(fid_host_feats)]    # stored as a list, as the reference does
        except Exception as e:
            print(f"  Warning: FID calculation failed: {e}")
    res = {"task": task_name, "num_samples": len(pairs), "metrics": {}}
    for k, vals in all_metrics.items():
        if vals:
            res["metrics"][k] = {"mean": np.mean(vals), "std": np.std(vals), "min": np.min(vals),
                                 "max": np.max(vals), "median": np.median(vals)}
    return res


def print_results(results: dict):
    print(f"\n{'=' * 60}")
    print(f"Evaluation Results: {results['task']}")
    print(f"{'=' * 60}")
    print(f"Number of samples: {results['num_samples']}")
    print("\nMetrics:")
    for name, st in results["metrics"].items():
        print(f"\n  {name.upper()}:")
        print(f"    Mean:   {st['mean']:.4f} ± {st['std']:.4f}")
        print(f"    Median: {st['median']:.4f}")
        print(f"    Range:  [{st['min']:.4f}, {st['max']:.4f}]")
    print(f"\n{'=' * 60}\n")
