"""Opt-in on-device image augmentation of the joint step (contract: include/cxrk.h, "augment").

`AugmentSpec` says WHAT is drawn (ranges; the default is the identity), `AugmentCall` is one call's descriptor (spec + the
(seed, counter, row offset) that select the draws).  The kernels are csrc/augment.hip; nothing here touches a tensor."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple


@dataclass(frozen=True)
class AugmentSpec:
    """Ranges of the random affine + photometric transform.  Per image: rotation uniform in +-rotate_deg, translation uniform in
    +-translate (a fraction of the output size, per axis), zoom log-uniform in [zoom[0], zoom[1]], horizontal flip with probability
    flip_p, brightness factor uniform in 1 +- brightness, contrast factor uniform in 1 +- contrast (about the image mean).
    out_size = (Ho, Wo): the size sampled to (None: the source size).  clamp01: clamp the result to [0, 1]."""
    rotate_deg: float = 0.0
    translate: float = 0.0
    zoom: Tuple[float, float] = (1.0, 1.0)
    flip_p: float = 0.0
    brightness: float = 0.0
    contrast: float = 0.0
    out_size: Optional[Tuple[int, int]] = None
    clamp01: bool = False

    def __post_init__(self):
        for name in ("rotate_deg", "translate", "flip_p", "brightness", "contrast"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"AugmentSpec.{name} must be a finite number, got {v!r}")
            object.__setattr__(self, name, float(v))
        try:
            lo, hi = (float(v) for v in self.zoom)
        except (TypeError, ValueError):
            raise ValueError(f"AugmentSpec.zoom must be a pair (lo, hi), got {self.zoom!r}") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
            raise ValueError(f"AugmentSpec.zoom needs finite 0 < lo <= hi, got {self.zoom!r}")
        object.__setattr__(self, "zoom", (lo, hi))
        if self.rotate_deg < 0 or self.translate < 0:
            raise ValueError(f"AugmentSpec: rotate_deg and translate are half-widths (>= 0), got {self.rotate_deg!r}, {self.translate!r}")
        if not 0.0 <= self.flip_p <= 1.0:
            raise ValueError(f"AugmentSpec.flip_p must lie in [0, 1], got {self.flip_p!r}")
        for name in ("brightness", "contrast"):
            v = getattr(self, name)
            if not 0.0 <= v < 1.0:
                raise ValueError(f"AugmentSpec.{name} must lie in [0, 1), got {v!r}")
        if self.out_size is not None:
            try:
                ho, wo = self.out_size
                ok = all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in (ho, wo))
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"AugmentSpec.out_size must be None or a pair of positive integers, got {self.out_size!r}")
            object.__setattr__(self, "out_size", (int(ho), int(wo)))
        object.__setattr__(self, "clamp01", bool(self.clamp01))

    @property
    def is_identity(self) -> bool:
        return (self.rotate_deg == 0 and self.translate == 0 and self.zoom == (1.0, 1.0) and self.flip_p == 0 and self.brightness == 0
                and self.contrast == 0 and not self.clamp01)

    def size_for(self, hs: int, ws: int) -> Tuple[int, int]:
        return (hs, ws) if self.out_size is None else self.out_size


# `drivers.py --joint --augment` / `Trainer(joint_encoders={"augment": True})`: no flip, laterality matters on chest films
DEFAULT_SPEC_ARGS = dict(rotate_deg=10.0, translate=0.05, zoom=(0.9, 1.1), flip_p=0.0, brightness=0.2, contrast=0.2)


def spec_from(value) -> Optional[AugmentSpec]:
    """None / False -> None; True -> the moderate default; a dict -> AugmentSpec(**dict); an AugmentSpec -> itself"""
    if value is None or value is False:
        return None
    if value is True:
        return AugmentSpec(**DEFAULT_SPEC_ARGS)
    if isinstance(value, AugmentSpec):
        return value
    if isinstance(value, dict):
        d = dict(value)
        for k in ("zoom", "out_size"):
            if d.get(k) is not None:
                d[k] = tuple(d[k])
        return AugmentSpec(**d)
    raise TypeError(f"augment: expected None, True, a dict of AugmentSpec fields or an AugmentSpec, got {type(value).__name__}")


class AugmentCall(NamedTuple):
    """One augmented forward: the draws of image i of the call are those of (seed, counter, row_offset + i)."""
    spec: AugmentSpec
    seed: int
    counter: int
    row_offset: int = 0
