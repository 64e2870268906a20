"""Rays for the quotient by T_origin in marchLoop (syzygy_amd/csrc/szg_device.hpp).

The lean loops divide the step's tap by the origin's (T_end / T_origin) on a ray that does not point up, and the other way
round on one that does; `up` is mu > 0, per lane. The divisor of the first form is the same at every step of a ray, so its
reciprocal need be formed only once per ray (the compiler hoists it today). Two kinds of family, built with
tests/march_rays.py and laid out with its layout():

* GATE: rays across mu = 0. Origin at 5 km altitude, path 0.05 Mm, vertical component 0, +-2^-149, +-2^-126, +-2^-60,
  +-2^-30, +-2^-24, +-2^-12, +-2^-4, +-0.3 and +-1.
  - "gate/sun-0.8": the origin where the sun cosine is 0.8 (ray64). In that frame the vertical is no coordinate axis and
    float32 keeps a vertical component only down to about 2^-24 of the direction's length: the smaller ones come out as
    whatever the rounding of the three components leaves, on either side of 0.
  - "gate/axis": the same components with the origin on the +y axis and the direction in the x-y plane, (sqrt(1 - v^2), v, 0):
    dot(origin, direction) is then the single product r * v, and the sign of every component, the denormal ones included,
    is the sign of mu. The sun cosine there is what the block's sun gives. This is the family the census counts.
  The rays with +-0.3 tap the LUT texel that the variant "lut-texel-2^-60" overwrites (row 9, column 14: the view taps at 5 km
  with |mu| = 0.3; T_origin is sampled at |mu|), on both sides of the gate.
* GRAZING: down rays from 1 m above the ground (r = Rp + 1e-6 Mm) with mu in [-0.02, 0], sun cosine 0.8, marched up to
  the ground hit - or, where mu is too flat to meet the ground (r^2 mu^2 < r^2 - Rp^2, |mu| < 5.6e-4), over 0.05 Mm. T_origin,
  the transmittance along such a ray to the top of the atmosphere, is the smallest divisor the march meets near the ground.
"""
import math

import numpy as np

from tests import march_rays as mr

VERTICALS = [0.0] + [s * v for v in (2.0 ** -149, 2.0 ** -126, 2.0 ** -60, 2.0 ** -30, 2.0 ** -24, 2.0 ** -12, 2.0 ** -4, 0.3, 1.0)
                     for s in (1.0, -1.0)]
ALTITUDE, PATH, SUN = 0.005, 0.05, 0.8
GRAZING_MU = [-x for x in np.geomspace(0.02, 0.0006, 16)] + [-5e-4, -2e-4, -1e-4, -1e-5, -1e-6, -1e-9, -0.0, 0.0]
# the wave's other lanes keep the lean loops with "inner" (the INNER prefix is lost) and lose them with "lean"
SPOILERS = ("inner", "lean")
VARIANTS = ("earth", "lut-texel-2^-60")


def axis_ray(B, v):
    return np.array([0.0, B.Rp + ALTITUDE, 0.0, math.sqrt(1.0 - v * v), v, 0.0, PATH])


def grazing_ray(B, mu):
    r = B.Rp + 1e-6
    disc = r * r * mu * mu - (r * r - B.Rp * B.Rp)
    D = (-r * mu - math.sqrt(disc)) if (mu < 0.0 and disc >= 0.0) else PATH
    return mr.ray64(B, r, mu, D, SUN)


def families(B, spoiler):
    """The three families, each with `spoiler` as the ray of its spoiled waves."""
    return [
        mr.Family("gate/sun-0.8", None, "points", list(VERTICALS), [mr.ray64(B, B.Rp + ALTITUDE, v, PATH, SUN) for v in VERTICALS], spoiler),
        mr.Family("gate/axis", None, "points", list(VERTICALS), [axis_ray(B, v) for v in VERTICALS], spoiler),
        mr.Family("grazing", None, "points", list(GRAZING_MU), [grazing_ray(B, mu) for mu in GRAZING_MU], spoiler),
    ]


def up64(ray, B):
    """MarchSetup::up of a float32 ray, by the float64 census."""
    return mr.census(ray, B)["q"]["mu"] > 0.0
