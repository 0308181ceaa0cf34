"""Training data for the SR generator (utils/datasets.py:274-355 SR_dataset).

The reference decodes, crops, resizes and normalises every sample on CPU
workers (cv2 + albumentations).  Here the CPU side only decodes and crops
(uint8, the smallest thing to move); resize to LR, Normalize and the HR
transform (PIL_to_tanh, utils/datasets.py:96-106, or Normalize for SRGAN
mode, :336-339) run batched on the GPU (`GPUTransform`).  `SyntheticSR`
generates smooth random HR crops directly on the GPU (no dataset is
available offline; SURVEY.md §8d's synthetic recipe).
"""
from __future__ import annotations

import ctypes
import json
import random
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import Dataset

from . import _lib, degrade, dihedral, ops

IMG_FORMATS = (".bmp", ".jpg", ".jpeg", ".png", ".tif", ".tiff", ".webp")
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def ground_up(x: int, factor: int) -> int:
    """utils/general.py ground_up: round x up to a multiple of factor."""
    return (x + factor - 1) // factor * factor


def list_images(src) -> list[str]:
    """A JSON list of paths (train.py:191 train_images.json) or a directory."""
    src = Path(src)
    if src.suffix == ".json":
        with open(src) as f:
            return [str(p) for p in json.load(f)]
    return sorted(str(p) for p in src.rglob("*") if p.suffix.lower() in IMG_FORMATS)


class SRCropDataset(Dataset):
    """Random `target_size` RGB crops as uint8 CHW (SR_dataset's RandomCrop,
    utils/datasets.py:288, 344-347); images smaller than the crop are padded."""

    def __init__(self, src, target_size: int, scale: int, prefix: str = ""):
        self.samples = list_images(src)
        if not self.samples:
            raise FileNotFoundError(f"no images under {src}")
        self.target_size = ground_up(target_size, scale)
        self.scale = scale
        print(f"{prefix}{len(self.samples)} images with target shape {self.target_size} with scale factor {scale}.")

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        from PIL import Image
        with Image.open(self.samples[i]) as im:
            a = np.asarray(im.convert("RGB"))
        t = self.target_size
        h, w = a.shape[:2]
        if h < t or w < t:
            a = np.pad(a, ((0, max(0, t - h)), (0, max(0, t - w)), (0, 0)), mode="reflect")
            h, w = a.shape[:2]
        y, x = random.randint(0, h - t), random.randint(0, w - t)
        return torch.from_numpy(np.ascontiguousarray(a[y:y + t, x:x + t])).permute(2, 0, 1).contiguous()


AUGMENTS = ("none", "flip", "dihedral")
AUGMENT_SEED_OFFSET = 0x0D4  # the augmentation generator's seed is the transform's `seed` plus this


class _Augment:
    """The geometric training augmentation GPUTransform and NoisyTransform share: per image one op of the
    dihedral group (dihedral.py), applied to the clean uint8 crops in ONE isr_dihedral launch before anything
    else.  "flip" draws k in {0, 4} (a mirror along the width or nothing), "dihedral" k uniform in 0..7
    (square crops only); each by exactly one torch.randint(0, 2 or 8, (n,), generator=self.gen, device=...)
    per call (x 4 for flip), never read back.  self.gen is a device generator of its own, seeded with
    seed + AUGMENT_SEED_OFFSET, so no other draw of the transform moves.  "none" draws and launches nothing."""

    def __init__(self, who: str, augment: str, seed: int, device):
        if augment not in AUGMENTS:
            raise ValueError(f"{who}: augment {augment!r} is not one of {', '.join(AUGMENTS)}")
        self.who, self.mode, self.device, self.gen = who, augment, device, None
        if augment != "none" and torch.device(device).type == "cuda":
            self.gen = torch.Generator(device=device).manual_seed(seed + AUGMENT_SEED_OFFSET)

    def __call__(self, crops_u8: torch.Tensor) -> torch.Tensor:
        if self.mode == "none":
            return crops_u8
        if self.gen is None:
            raise RuntimeError(f"{self.who}: augment={self.mode!r} is a HIP kernel (MI355X only); device "
                               f"{self.device!r} has no such path (there is no host fallback)")
        x = degrade._checked(crops_u8, self.who, on_device=False).to(self.device, non_blocking=True)
        if self.mode == "dihedral" and x.shape[-2] != x.shape[-1]:
            raise ValueError(f"{self.who}: augment='dihedral' turns crops by 90 degrees and needs square ones, got "
                             f"{x.shape[-2]}x{x.shape[-1]} (augment='flip' takes any shape)")
        n = x.shape[0]
        if self.mode == "flip":
            ids = torch.randint(0, 2, (n,), generator=self.gen, device=x.device).to(torch.int32) * 4
            if x.shape[-2] != x.shape[-1]:
                # a mirror along the width keeps the shape, but per-image ops are for square batches: flip
                # every image into a second batch (one launch) and let the ids choose
                return torch.where((ids != 0).view(n, 1, 1, 1), dihedral.apply(x, 4), x)
        else:
            ids = torch.randint(0, 8, (n,), generator=self.gen, device=x.device).to(torch.int32)
        return dihedral.apply(x, ids)


class GPUTransform:
    """Batched (hr, lr) from uint8 HR crops on the device:
    lr = Normalize(Resize(crop, T/scale)) (albumentations Resize = cv2 INTER_LINEAR,
    utils/datasets.py:302-303); hr = 2*crop/255 - 1 (PIL_to_tanh) or
    Normalize(crop) when hr_norm (set_transform_hr, SRGAN mode).

    cv2 resizes the uint8 image and returns uint8: at the integer factors train.py uses
    (2, 3, 4) its fixed-point INTER_LINEAR (11-bit coefficients; x2 runs as INTER_AREA)
    samples at src = scale*(d + 0.5) - 0.5 with weights 0 / 0.5 / 1, i.e. the exact float
    bilinear value rounded half up — reproduced here by rounding the float interpolation
    of the uint8 values (oracle.ref_cpu.cv2_resize_linear_u8 restates the fixed-point
    arithmetic; tests/test_data_cpu.py).

    `lr_filter` chooses the LR model.  "cv2" (the default) is the above, SR_dataset's.  A name of
    degrade.RESAMPLE_FILTERS ("bicubic", ...) makes the LR with Pillow's antialiased Image.resize
    instead, bit for bit (Random_low_rs, utils/datasets.py:23-32), hr and lr still in ONE launch
    (isr_resample_u8).  "random" is image_reader's mix (:218-246): per image one of RANDOM_FILTERS
    = (bicubic, bilinear, box, nearest), each with probability 0.25, drawn by exactly one
    torch.randint(0, 4, (n,), generator=self.gen, device=...) per call (self.gen seeded with
    `seed`) and never read back.  These are HIP kernels: on a CPU device they raise.

    `degrade` (an LRDegrade, or None) degrades a copy of the crops before the resize, with every
    lr_filter: hr is made from the clean crops and is bit for bit what it is without `degrade`;
    lr is the same resize + Normalize of the degraded copy (one more launch of the transform's
    kernel).  The `random` draw above happens before the degradation's draws and from a generator
    of its own, so it is the same with and without `degrade`; with every probability 0 lr is
    unchanged too.  HIP only.

    `augment` ("none", "flip" or "dihedral": _Augment) transforms the clean crops first, ahead of `degrade` and
    of both resizes, so hr and lr show the same transformed picture; its ids come from a generator of its
    own (seed + AUGMENT_SEED_OFFSET), so the `random` filter draw and the degradation's draws are the same
    with and without it.  "none" (the default) launches nothing and changes no output bit.  HIP only."""

    LR_FILTERS = ("cv2", "nearest", "box", "bilinear", "hamming", "bicubic", "lanczos", "random")
    RANDOM_FILTERS = ("bicubic", "bilinear", "box", "nearest")

    def __init__(self, scale: int, hr_norm: bool = False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda",
                 lr_filter: str = "cv2", seed: int = 0, degrade: "LRDegrade | None" = None,
                 augment: str = "none"):
        self.augment = _Augment("GPUTransform", augment, seed, device)
        if lr_filter not in self.LR_FILTERS:
            raise ValueError(f"GPUTransform: lr_filter {lr_filter!r} is not one of {', '.join(self.LR_FILTERS)}")
        self.scale, self.hr_norm = scale, hr_norm
        self.degrade = degrade
        self.lr_filter, self.seed, self.gen = lr_filter, seed, None
        if lr_filter == "random" and torch.device(device).type == "cuda":
            self.gen = torch.Generator(device=device).manual_seed(seed)
        self.mean = torch.tensor(mean, device=device).view(1, 3, 1, 1)
        self.std = torch.tensor(std, device=device).view(1, 3, 1, 1)
        self.mean_f, self.std_f = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.device = device

    def __call__(self, crops_u8: torch.Tensor):
        """(hr, lr).  The two kernels are backends of one call shape, (x, want_hr, want_lr) -> (hr, lr)."""
        on_gpu = torch.device(self.device).type == "cuda"
        if self.lr_filter != "cv2" and not on_gpu:
            raise RuntimeError(f"GPUTransform: lr_filter={self.lr_filter!r} is a HIP kernel (MI355X only); device "
                               f"{self.device!r} has no such path (there is no host fallback)")
        if self.lr_filter == "cv2" and not on_gpu and self.degrade is None and self.augment.mode == "none":
            return self._cv2_on_cpu(crops_u8)
        x = self.augment(self._crops(crops_u8))
        backend = self._cv2 if self.lr_filter == "cv2" else self._pillow(x)
        if self.degrade is None:
            return backend(x, True, True)
        # hr from the clean crops, lr from the degraded copy (one more launch of the backend's kernel)
        degraded = self.degrade(x)
        return backend(x, True, False)[0], backend(degraded, False, True)[1]

    def _cv2_on_cpu(self, crops_u8: torch.Tensor):
        """CPU device: the cv2 formulas as torch ops (host-side tests; the GPU path is the kernel)."""
        x255 = crops_u8.to(self.device, non_blocking=True).float()
        t = x255.shape[-1]
        lr = F.interpolate(x255, size=(t // self.scale, t // self.scale), mode="bilinear", align_corners=False,
                           antialias=False)
        lr = (lr + 0.5).floor_().div_(255.0)  # cv2's uint8 result (round half up), then /255
        lr = (lr - self.mean) / self.std
        x = x255.div_(255.0)
        hr = (x - self.mean) / self.std if self.hr_norm else x * 2.0 - 1.0
        return hr.contiguous(), lr.contiguous()

    def _crops(self, crops_u8: torch.Tensor) -> torch.Tensor:
        """The checked crops on the device: uint8 [n, 3, t, t], t a multiple of the scale."""
        degrade._checked(crops_u8, "GPUTransform", on_device=False)
        t, tw = crops_u8.shape[-2:]
        if t != tw or t % self.scale:
            raise ValueError(f"GPUTransform: square crops with side a multiple of {self.scale}, got {t}x{tw}")
        return crops_u8.to(self.device, non_blocking=True).contiguous()

    def _cv2(self, x: torch.Tensor, want_hr: bool, want_lr: bool):
        """One HIP launch (isr_sr_transform): crop block reads, cv2 resize, both Normalizes.  The kernel
        has no optional outputs: both are made whatever is wanted."""
        n, _, t, _ = x.shape
        hr = torch.empty((n, 3, t, t), device=x.device)
        lr = torch.empty((n, 3, t // self.scale, t // self.scale), device=x.device)
        d = _lib.IsrSrTransformDesc(x.data_ptr(), hr.data_ptr(), lr.data_ptr(), n, t, self.scale,
                                    int(self.hr_norm), (ctypes.c_float * 3)(*self.mean_f),
                                    (ctypes.c_float * 3)(*self.std_f))
        _lib.check(_lib.load().isr_sr_transform(ctypes.byref(d), ops._stream()), "isr_sr_transform")
        return hr, lr

    def _pillow(self, x: torch.Tensor):
        """The Pillow backend of one call, one HIP launch each time it runs (isr_resample_u8: the resize to
        LR, both Normalizes, the HR tensor).  `random`'s filter ids are drawn here, once per call."""
        if self.lr_filter == "random":
            names = self.RANDOM_FILTERS
            ids = torch.randint(0, 4, (x.shape[0],), generator=self.gen, device=x.device).to(torch.int32)
        else:
            names, ids = (self.lr_filter,), None
        filters = tuple(degrade.RESAMPLE_FILTERS.index(f) for f in names)
        size = (x.shape[-1] // self.scale,) * 2

        def backend(x, want_hr, want_lr):
            _, lr, hr = degrade.resample_launch(x, size, filters, ids, want_lr=want_lr, want_hr=want_hr,
                                                hr_norm=self.hr_norm, mean=self.mean_f, std=self.std_f)
            return hr, lr
        return backend


def _jpeg_range(jpeg_quality, who: str) -> tuple[int, int]:
    lo, hi = jpeg_quality
    if int(lo) != lo or int(hi) != hi or not 1 <= lo <= hi <= 100:
        raise ValueError(f"{who}: jpeg quality range must be integers with 1 <= lower <= upper <= 100, "
                         f"got {jpeg_quality}")
    return int(lo), int(hi)


# The per-image stages NoisyTransform and LRDegrade share.  Their draws from `gen`, in this order, are
# part of both classes' contracts (the class docstrings; tests/test_gpu_degrade_draws.py).

def _iso_stage(u8: torch.Tensor, gen, p: float, color_shift_range, intensity_range) -> torch.Tensor:
    """ISONoise: rand(n) < p, uniform(n) colour shift, uniform(n) intensity, then degrade.iso_noise's draws."""
    n, dev = u8.shape[0], u8.device
    on = torch.rand(n, device=dev, generator=gen) < p
    cs = torch.empty(n, device=dev).uniform_(*color_shift_range, generator=gen)
    it = torch.empty(n, device=dev).uniform_(*intensity_range, generator=gen)
    return degrade.iso_noise(u8, cs, it, gen, apply=on)


def _jpeg_stage(u8: torch.Tensor, gen, p: float, quality_range) -> torch.Tensor:
    """ImageCompression: rand(n) < p, randint(n) in the inclusive range; quality 0 copies an image through."""
    n, dev = u8.shape[0], u8.device
    on = torch.rand(n, device=dev, generator=gen) < p
    lo, hi = quality_range
    q = torch.randint(int(lo), int(hi) + 1, (n,), device=dev, generator=gen, dtype=torch.int32)
    return degrade.jpeg_roundtrip(u8, q * on.to(torch.int32))


def _gauss_noise(shape, n: int, gen, device, var_limit, p: float) -> torch.Tensor:
    """GaussNoise's additive term on the 0-255 scale: uniform(n, 1, 1, 1) variance, rand(n, 1, 1, 1) < p,
    randn(shape)."""
    var = torch.empty(n, 1, 1, 1, device=device).uniform_(*var_limit, generator=gen)
    on = (torch.rand(n, 1, 1, 1, device=device, generator=gen) < p).float()
    return torch.randn(shape, device=device, generator=gen) * var.sqrt() * on


class NoisyTransform:
    """Batched (clean, noisy) pairs for `train.py --train_denoise` from uint8 crops
    on the device (Noisy_dataset, utils/datasets.py:361-389): clean = 2*crop/255 - 1;
    noisy = Normalize(ImageCompression(ISONoise(GaussNoise(crop)))), each stage applied per
    sample with its own probability:

    * GaussNoise, albumentations defaults: var_limit (10, 50) on the 0-255 scale, per channel,
      probability `p`, result clipped to [0, 255];
    * ISONoise (probability `iso_p`): Poisson luminance and Gaussian hue noise in HLS space,
      color_shift and intensity uniform in `iso_color_shift` / `iso_intensity`
      (degrade.iso_noise, libisr's isr_hls_l_moments + isr_iso_noise);
    * ImageCompression (probability `jpeg_p`): a JPEG round trip at an integer quality uniform
      in the inclusive `jpeg_quality` range (degrade.jpeg_roundtrip, libisr's isr_jpeg_roundtrip).

    With iso_p = jpeg_p = 0 (the default) only GaussNoise runs, in float, and the output and the
    generator's draws are what they were before the other stages existed.  With either on, the
    stages exchange uint8 images as the reference's do (GaussNoise's result is truncated to
    uint8), the extra draws follow the three GaussNoise draws, and the stages are HIP kernels:
    a CPU device raises.  `NoisyTransform.reference(...)` is the reference's pipeline
    (iso_p = jpeg_p = 0.5).

    `augment` ("none", "flip" or "dihedral": _Augment) transforms the uint8 crops before all of the above,
    so clean and noisy show the same transformed picture; its ids come from a generator of its own
    (seed + AUGMENT_SEED_OFFSET), so the noise draws are the same with and without it.  "none" (the
    default) launches nothing.  HIP only."""

    def __init__(self, mean=IMAGENET_MEAN, std=IMAGENET_STD, var_limit=(10.0, 50.0), p: float = 0.5,
                 device="cuda", seed: int = 0, iso_p: float = 0.0, jpeg_p: float = 0.0, jpeg_quality=(50, 75),
                 iso_color_shift=(0.01, 0.05), iso_intensity=(0.1, 0.5), augment: str = "none"):
        self.augment = _Augment("NoisyTransform", augment, seed, device)
        self.mean = torch.tensor(mean, device=device).view(1, 3, 1, 1)
        self.std = torch.tensor(std, device=device).view(1, 3, 1, 1)
        self.var_limit, self.p, self.device = var_limit, p, device
        self.iso_p, self.jpeg_p = float(iso_p), float(jpeg_p)
        self.jpeg_quality, self.iso_color_shift, self.iso_intensity = jpeg_quality, iso_color_shift, iso_intensity
        _jpeg_range(jpeg_quality, "NoisyTransform")
        self.gen = torch.Generator(device=device).manual_seed(seed)

    @classmethod
    def reference(cls, *args, **kw):
        """The reference's Noisy_dataset pipeline: all three stages at p = 0.5."""
        kw.setdefault("iso_p", 0.5)
        kw.setdefault("jpeg_p", 0.5)
        return cls(*args, **kw)

    def __call__(self, crops_u8: torch.Tensor):
        x = self.augment(crops_u8).to(self.device, non_blocking=True).float()
        noise = _gauss_noise(x.shape, x.shape[0], self.gen, self.device, self.var_limit, self.p)
        hr = x / 255.0 * 2.0 - 1.0
        if self.iso_p > 0 or self.jpeg_p > 0:
            # ISONoise and the JPEG round trip on the uint8 result of GaussNoise (HIP only)
            if torch.device(self.device).type != "cuda":
                raise RuntimeError("NoisyTransform: the ISONoise and JPEG stages are HIP kernels (MI355X only); "
                                   f"device {self.device!r} has no such path (there is no host fallback)")
            u8 = (x + noise).clamp_(0, 255).to(torch.uint8)
            if self.iso_p > 0:
                u8 = _iso_stage(u8, self.gen, self.iso_p, self.iso_color_shift, self.iso_intensity)
            if self.jpeg_p > 0:
                u8 = _jpeg_stage(u8, self.gen, self.jpeg_p, self.jpeg_quality)
            noisy = u8.float().div_(255.0)
        else:
            noisy = (x + noise).clamp_(0, 255).div_(255.0)
        lr = (noisy - self.mean) / self.std
        return hr.contiguous(), lr.contiguous()


class LRDegrade:
    """The blind-SR degradation of the HR crops that the LR image is then resized from: the stages
    the reference lists, commented out, ahead of SR_dataset.transform_lr's Resize
    (utils/datasets.py:291-305), in its order, each applied per image with its own probability,
    exchanging uint8 [n, 3, t, t] images:

    1. ISONoise (`iso_p`; color_shift / intensity uniform in `iso_color_shift` / `iso_intensity`);
    2. ImageCompression (`jpeg_p`; a JPEG round trip at an integer quality uniform in the inclusive
       `jpeg_quality`; the crop side must then be a multiple of 16);
    3. blur (`blur_p`): ONE draw among `blur_kinds` ("box", "gaussian", "motion", "median", uniform)
       with k uniform in `blur_ksizes` (default 3, 5, 7) — not the reference's four independent
       stages Blur, GaussianBlur, MotionBlur and MedianBlur, whose probabilities `blind` sums.
       Gaussian: sigma_x, sigma_y uniform in [0.2, 3.0], angle in [0, pi); motion: a line between
       two points of the k x k grid drawn as albumentations' MotionBlur draws them;
    4. GaussNoise (`gauss_p`; variance uniform in `var_limit` on the 0-255 scale, per channel, the
       result clipped and truncated to uint8).

    The input is not written to.  All four are HIP kernels or device tensor ops (degrade.iso_noise,
    jpeg_roundtrip, blur_u8): a CPU tensor raises.  Nothing is read back from the device.

    Draws.  Stages 1, 2 and 4 draw from a device generator seeded with `seed`, as NoisyTransform
    does, and only when their probability is > 0: ISONoise rand(n), uniform(n) color shift,
    uniform(n) intensity, then degrade.iso_noise's poisson(n, t, t) and randn(n, t, t); JPEG rand(n),
    randint(n); GaussNoise uniform(n, 1, 1, 1), rand(n, 1, 1, 1), randn(n, 3, t, t).  The blur stage
    draws on the HOST from a CPU generator seeded with `seed`, when blur_p > 0, exactly five float64 /
    int64 tensors per call, whatever is applied:
        a = torch.rand(n)            apply where a < blur_p
        b = torch.randint(0, len(blur_kinds), (n,))   the kind, an index into blur_kinds
        c = torch.randint(0, len(blur_ksizes), (n,))  k = blur_ksizes[c]
        g = torch.rand(n, 3)         sigma_x = 0.2 + 2.8 g0, sigma_y = 0.2 + 2.8 g1, angle = pi g2
        m = torch.rand(n, 4)         x1 = floor(k m0), x2 = floor(k m1), y1 = floor(k m2), and
                                     y2 = floor(k m3) if x1 != x2 else (y1 + 1 + floor((k - 1) m3)) mod k
    (`blur_params` is that, as plain Python).  The [n, 49] tap table is built by libisr's host code
    (degrade.blur_taps) and goes up in one non-blocking copy from pinned memory.  One motion draw has
    no table: a six-pixel line (k = 7) that misses the centre pixel rounds to taps summing to 65538,
    which isr_blur_taps refuses; that image is left unblurred."""

    BLUR_KINDS = ("box", "gaussian", "motion", "median")

    def __init__(self, iso_p: float = 0.0, jpeg_p: float = 0.0, jpeg_quality=(45, 75), blur_p: float = 0.0,
                 blur_kinds=BLUR_KINDS, gauss_p: float = 0.0, var_limit=(10.0, 50.0), iso_color_shift=(0.01, 0.05),
                 iso_intensity=(0.1, 0.5), seed: int = 0, device="cuda", blur_ksizes=(3, 5, 7)):
        blur_kinds, blur_ksizes = tuple(blur_kinds), tuple(int(k) for k in blur_ksizes)
        if not blur_ksizes or any(k not in (3, 5, 7) for k in blur_ksizes):
            raise ValueError(f"LRDegrade: blur_ksizes {blur_ksizes!r} must be a non-empty choice of 3, 5 and 7")
        if not blur_kinds or any(k not in self.BLUR_KINDS for k in blur_kinds):
            raise ValueError(f"LRDegrade: blur_kinds {blur_kinds!r} must be a non-empty subset of {self.BLUR_KINDS}")
        jpeg_quality = _jpeg_range(jpeg_quality, "LRDegrade")
        for name, p in (("iso_p", iso_p), ("jpeg_p", jpeg_p), ("blur_p", blur_p), ("gauss_p", gauss_p)):
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"LRDegrade: {name} = {p} is not a probability")
        self.iso_p, self.jpeg_p, self.blur_p, self.gauss_p = float(iso_p), float(jpeg_p), float(blur_p), float(gauss_p)
        self.jpeg_quality, self.blur_kinds, self.var_limit = jpeg_quality, blur_kinds, var_limit
        self.blur_ksizes = blur_ksizes
        self.iso_color_shift, self.iso_intensity = iso_color_shift, iso_intensity
        self.seed, self.device = seed, device
        self.gen = torch.Generator(device=device).manual_seed(seed)
        self.host_gen = torch.Generator(device="cpu").manual_seed(seed)

    PRESETS = {
        # the blur stage alone
        "blur": dict(blur_p=0.5),
        # the probabilities of the reference's commented list (ISONoise 0.05, ImageCompression 0.1 at quality
        # 45..75, Blur + GaussianBlur + MotionBlur + MedianBlur 0.05 + 0.1 + 0.1 + 0.05, GaussNoise 0.1)
        "blind": dict(iso_p=0.05, jpeg_p=0.1, jpeg_quality=(45, 75), blur_p=0.3, gauss_p=0.1),
    }

    @classmethod
    def preset(cls, name: str, **kw):
        """`train.py --lr_degrade`'s chains: "blur" or "blind" (PRESETS)."""
        if name not in cls.PRESETS:
            raise ValueError(f"LRDegrade: unknown preset {name!r}; one of {', '.join(cls.PRESETS)}")
        return cls(**cls.PRESETS[name], **kw)

    @staticmethod
    def blur_params(n: int, blur_p: float, blur_kinds, gen: torch.Generator, blur_ksizes=(3, 5, 7)) -> list[dict]:
        """The blur stage's host draws of one call of n images from the CPU generator `gen` (the
        class docstring's five tensors), decoded: per image a dict with `apply`, `kind`, `ksize`
        and, for gaussian and motion, `params` (degrade.blur_taps' keywords)."""
        import math
        a = torch.rand(n, generator=gen, dtype=torch.float64).tolist()
        b = torch.randint(0, len(blur_kinds), (n,), generator=gen).tolist()
        c = torch.randint(0, len(blur_ksizes), (n,), generator=gen).tolist()
        g = torch.rand(n, 3, generator=gen, dtype=torch.float64).tolist()
        m = torch.rand(n, 4, generator=gen, dtype=torch.float64).tolist()
        out = []
        for i in range(n):
            k, kind = blur_ksizes[c[i]], blur_kinds[b[i]]
            rec = dict(apply=a[i] < blur_p, kind=kind, ksize=k, params={})
            if kind == "gaussian":
                rec["params"] = dict(sigma_x=0.2 + 2.8 * g[i][0], sigma_y=0.2 + 2.8 * g[i][1], angle=math.pi * g[i][2])
            elif kind == "motion":
                x1, x2, y1 = (min(int(k * v), k - 1) for v in m[i][:3])
                y2 = min(int(k * m[i][3]), k - 1) if x1 != x2 else (y1 + 1 + min(int((k - 1) * m[i][3]), k - 2)) % k
                rec["params"] = dict(x1=x1, y1=y1, x2=x2, y2=y2)
            out.append(rec)
        return out

    def __call__(self, crops_u8: torch.Tensor) -> torch.Tensor:
        u8 = degrade._checked(crops_u8, "LRDegrade", on_device=False)
        n, (h, w) = u8.shape[0], u8.shape[-2:]
        if self.jpeg_p > 0 and (h % 16 or w % 16):
            raise ValueError(f"LRDegrade: jpeg_p = {self.jpeg_p} needs whole 16 x 16 MCUs, but the crop is {h}x{w}: "
                             "choose a crop side that is a multiple of 16, or jpeg_p = 0")
        if not u8.is_cuda or torch.device(self.device).type != "cuda":
            raise RuntimeError("LRDegrade: the degradations are HIP kernels (MI355X only); got a tensor on "
                               f"{u8.device} for device {self.device!r} (there is no host fallback)")
        if self.iso_p > 0:
            u8 = _iso_stage(u8, self.gen, self.iso_p, self.iso_color_shift, self.iso_intensity)
        if self.jpeg_p > 0:
            u8 = _jpeg_stage(u8, self.gen, self.jpeg_p, self.jpeg_quality)
        if self.blur_p > 0:
            u8 = self._blur(u8)
        if self.gauss_p > 0:
            noise = _gauss_noise(u8.shape, n, self.gen, u8.device, self.var_limit, self.gauss_p)
            u8 = (u8.float() + noise).clamp_(0, 255).to(torch.uint8)
        return u8

    def _blur(self, u8: torch.Tensor) -> torch.Tensor:
        """The blur stage: host draws, host-built tables, one isr_blur_u8 launch."""
        n = u8.shape[0]
        # one pinned block per call: [n][49 taps, ksize, median]; ksize 0 copies the image through
        host = torch.zeros((n, 51), dtype=torch.int32).pin_memory()
        for i, rec in enumerate(self.blur_params(n, self.blur_p, self.blur_kinds, self.host_gen,
                                                    self.blur_ksizes)):
            if not rec["apply"]:
                continue
            host[i, 49] = rec["ksize"]
            if rec["kind"] == "median":
                host[i, 50] = 1
            else:
                try:
                    taps = degrade.blur_taps(rec["kind"], rec["ksize"], **rec["params"])
                except _lib.IsrError:  # the refused motion line (class docstring): the image stays as it is
                    host[i, 49] = 0
                    continue
                host[i, :49] = torch.from_numpy(taps.reshape(49))
        dev = host.to(u8.device, non_blocking=True)
        return degrade.blur_u8(u8, dev[:, 49], dev[:, 50], dev[:, :49].reshape(n, 7, 7))


NATURAL_ALPHA = 1.4  # amplitude spectrum 1/f^alpha: x4 bicubic PSNR ~27.7 dB, the regime of COCO crops


def natural_hr_u8(n: int, t: int, generator: torch.Generator, device="cuda", alpha: float = NATURAL_ALPHA,
                  contrast: float = 0.25) -> torch.Tensor:
    """uint8 [n, 3, t, t] Gaussian fields with a natural-image power spectrum.

    White noise (a luma field shared by the channels plus 0.35x independent colour noise) shaped
    by 1/f^alpha in the Fourier domain, unit standard deviation per image, mapped to
    0.5 + contrast*x and clipped to [0, 1].  At alpha = 1.4 the x4 task is as hard as natural
    photos are for bicubic upsampling (about 27.7 dB PSNR on the cv2 LR of train.py), unlike the
    smooth kind, where bicubic already reaches ~46 dB and the last bf16 bits never matter."""
    w = torch.randn(n, 3, t, t, generator=generator, device=device)
    luma = torch.randn(n, 1, t, t, generator=generator, device=device)
    w = 0.35 * w + luma
    fy = torch.fft.fftfreq(t, device=device).view(-1, 1)
    fx = torch.fft.rfftfreq(t, device=device).view(1, -1)
    f = torch.sqrt(fx * fx + fy * fy).clamp_min(1.0 / t)
    x = torch.fft.irfft2(torch.fft.rfft2(w) / f.pow(alpha), s=(t, t))
    x = x / x.flatten(1).std(1).view(-1, 1, 1, 1)
    return (0.5 + contrast * x).clamp_(0, 1).mul_(255).round_().to(torch.uint8)


def leaves_hr_u8(n: int, t: int, generator: torch.Generator, device="cuda", discs: int = 500, rmin: float = 4.0,
                  contrast: float = 0.6, texture: float = 0.3) -> torch.Tensor:
    """uint8 [n, 3, t, t] 'dead leaves' images: the standard synthetic model of natural-image
    statistics (occluding objects with a power-law size distribution give sharp edges and a
    1/f-like spectrum), plus a 1/f^1.4 texture (natural_hr_u8) on top.

    `discs` opaque discs per image, front to back: centre uniform over the image, radius
    r ~ r^-3 on [rmin, t/3], a uniform random RGB colour; every pixel shows the first disc that
    covers it (grey where none does); colours enter as 0.5 + contrast*(c - 0.5), the texture as
    texture*(its [0, 1] value - 0.5).  x4 bicubic on these reaches ~27 dB, a trained x4 RRDB
    generator a few dB more (edges are what SR recovers; a Gaussian field has none)."""
    ys = torch.arange(t, dtype=torch.float32, device=device).view(1, t, 1)
    xs = torch.arange(t, dtype=torch.float32, device=device).view(1, 1, t)
    rmax, a1 = t / 3.0, -2.0  # 1 - alpha for alpha = 3
    out = torch.empty(n, 3, t, t, device=device)
    for i in range(n):
        cy = torch.rand(discs, generator=generator, device=device) * t
        cx = torch.rand(discs, generator=generator, device=device) * t
        u = torch.rand(discs, generator=generator, device=device)
        r2 = ((rmin ** a1 + u * (rmax ** a1 - rmin ** a1)) ** (1.0 / a1)) ** 2
        col = 0.5 + contrast * (torch.rand(discs, 3, generator=generator, device=device) - 0.5)
        top = torch.full((t, t), discs, dtype=torch.long, device=device)  # index of the top disc
        for j0 in range(0, discs, 64):  # front to back: a pixel keeps the first disc that covers it
            sl = slice(j0, min(j0 + 64, discs))
            inside = (ys - cy[sl].view(-1, 1, 1)) ** 2 + (xs - cx[sl].view(-1, 1, 1)) ** 2 <= r2[sl].view(-1, 1, 1)
            first = inside.to(torch.uint8).argmax(0) + j0
            top = torch.where(inside.any(0) & (top == discs), first, top)
        pal = torch.cat([col, torch.full((1, 3), 0.5, device=device)])
        out[i] = pal[top].permute(2, 0, 1)
    tex = natural_hr_u8(n, t, generator, device).float().div_(255.0).sub_(0.5)
    return (out + texture * tex).clamp_(0, 1).mul_(255).round_().to(torch.uint8)


class SyntheticSR:
    """Endless synthetic uint8 HR crops on the GPU, seed per batch and rank.

    kind "smooth": bicubic-upsampled 32x32 uniform noise (a smooth 'natural-ish' image);
    kind "natural": 1/f^1.4 Gaussian fields (natural_hr_u8);
    kind "leaves": dead-leaves images with a 1/f texture (leaves_hr_u8), the data the committed
    trained weights (tests/golden/trained_resnet_x4.safetensors) were made from."""

    def __init__(self, batch: int, target_size: int, seed: int = 0, device="cuda", kind: str = "smooth"):
        if kind not in ("smooth", "natural", "leaves"):
            raise ValueError(f"SyntheticSR kind {kind!r}: 'smooth', 'natural' or 'leaves'")
        self.batch, self.t, self.seed, self.device, self.kind = batch, target_size, seed, device, kind
        self.i = 0

    def __iter__(self):
        return self

    def __next__(self) -> torch.Tensor:
        g = torch.Generator(device=self.device).manual_seed(self.seed * 1_000_003 + self.i)
        self.i += 1
        if self.kind == "natural":
            return natural_hr_u8(self.batch, self.t, g, self.device)
        if self.kind == "leaves":
            return leaves_hr_u8(self.batch, self.t, g, self.device)
        base = torch.rand(self.batch, 3, 32, 32, generator=g, device=self.device)
        hr = F.interpolate(base, size=(self.t, self.t), mode="bicubic", align_corners=False).clamp_(0, 1)
        return (hr * 255).round_().to(torch.uint8)
