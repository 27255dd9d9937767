"""What PreissmannBatch.route_pool routes a boundary's inflow through: a reservoir as data.

PoolSpec restates what GerdHydrograph.build (cases/gerd_roseires/gerd_discharge.py:12-56) carries in its code - the volume curve it
reads, the weirs and the turbine flow of effective_capacity (:70-94), the 1e-6 that turns m3 into the curve's unit and brentq's
bracket - so that the device can route every member of an ensemble through a pool of its own.  No arithmetic happens here."""
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

from . import _pack as P


@dataclass(frozen=True)
class PoolSpec:
    """curve_stage [K] (increasing) / curve_volume [K]: the pool's volume over its stage; weirs: rows of (C, crest) or
    (C, crest, ramp_top) with Q = C * max(0, z - crest)^1.5, opened linearly from 0 at the crest to 1 at ramp_top; base_flow: what is
    always released (the turbines); vol_scale: m3 -> the curve's unit; z_lo, z_hi: the bracket every level's stage is sought in."""
    curve_stage: Sequence[float]
    curve_volume: Sequence[float]
    weirs: Sequence[Tuple[float, ...]]
    base_flow: float
    vol_scale: float
    z_lo: float
    z_hi: float

    def __post_init__(self):
        P.pool_descriptor(self.curve_stage, self.curve_volume, self.weirs)      # raises what the library would refuse
        if not self.z_lo < self.z_hi:
            raise ValueError("the bracket needs z_lo < z_hi")
        if not (self.base_flow >= 0 and self.vol_scale > 0):
            raise ValueError("base_flow >= 0 and vol_scale > 0 required")

    def arrays(self):
        """(curve_stage, curve_volume, weirs [n_w, 4]) as the C ABI takes them"""
        return P.pool_descriptor(self.curve_stage, self.curve_volume, self.weirs)

    def without_weir(self, w):
        ws = [tuple(x) for i, x in enumerate(self.weirs) if i != w]
        return PoolSpec(np.asarray(self.curve_stage), np.asarray(self.curve_volume), ws, self.base_flow, self.vol_scale, self.z_lo, self.z_hi)
