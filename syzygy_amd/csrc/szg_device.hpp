// szg_device.hpp — device-side math shared by the CDNA4 kernels.
//
// Every function keeps the operation ORDER of the GLSL it implements (cited
// per function, paths relative to the reference's shaders/ directory) so that
// with -ffp-contract=off the +,-,*,/,sqrt results are bit-identical to a
// straight evaluation; exp/pow/sin/cos/asin/acos are the pinned fp32 algorithms
// of include/szg/fpmath.h (never the device math library), so the kernels
// reproduce the scalar oracle bit for bit.
// What differs from the shaders is purely structural: loop invariants are
// hoisted into per-ray / per-light / per-atmosphere constants, images are
// linear buffers, samplers are explicit address arithmetic.
//
// The code lives in one header per subject; this one includes them all, for the test kernels and the measurement tools.
// The product's units include the headers they use.
#pragma once

#include "szg_vec.hpp"        // V2 / V3 / V4, M4 and their operators under the contraction rule
#include "szg_lean.hpp"       // the lean exact operators (rcpN, divR, sqrtN, expInner, powLean) and waveAll
#include "szg_formats.hpp"    // store formats and image views
#include "szg_atmosphere.hpp" // the atmosphere block, extinction, the transmittance-LUT samplers, FramePrep
#include "szg_march.hpp"      // phase functions and the 32-step scattering integral
#include "szg_pbr.hpp"        // materials, the BRDF, shadow-map sampling
