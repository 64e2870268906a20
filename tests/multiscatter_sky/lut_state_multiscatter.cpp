// lut_state_multiscatter.cpp — host only, no HIP: the events that include/szg/multiscatter_sky.h adds to the LUT bookkeeping of
// the sky-view pipeline (syzygy_amd/csrc/lut_state.hpp), walked one by one. tests/test_lut_state_multiscatter.py compiles this
// with g++ and runs it; tests/cpp/lut_state.cpp walks the events that were there before. FS is forceSkyview, P is
// multiscatterPresent; the other flags of the state must not move.
#include <cstdio>

#include "lut_state.hpp"

using szg::LutState;

static int failures = 0;
#define CHECK(cond)                                                                                                            \
    do                                                                                                                         \
    {                                                                                                                          \
        if (!(cond))                                                                                                           \
        {                                                                                                                      \
            printf("line %d: %s\n", __LINE__, #cond);                                                                          \
            failures++;                                                                                                        \
        }                                                                                                                      \
    } while (0)

constexpr uint32_t HEIGHT = 32u;

// both LUTs valid, nothing forced, no multi-scattering LUT yet
static LutState settled()
{
    LutState s;
    s.transmittance_recorded();
    s.skyview_rows_recorded(0u, HEIGHT, HEIGHT);
    return s;
}
// FS and P as given, and every older flag as settled() leaves it
static bool is(const LutState& s, bool FS, bool P)
{
    return s.forceSkyview == FS && s.multiscatterPresent == P && s.tlutStatusValid && s.slutStatusValid && !s.sliceStatusKnown &&
           !s.forceTransmittance;
}

int main()
{
    CHECK(!LutState{}.multiscatterPresent && is(settled(), false, false));
    {
        LutState s = settled(); // a change of mode: the texels are another function now
        s.multiscatter_mode_changed();
        CHECK(is(s, true, false));
        s.skyview_rows_recorded(0u, HEIGHT, HEIGHT);
        CHECK(is(s, false, false));
    }
    {
        LutState s = settled(); // recorded by the library: present, nothing forced, whatever the mode
        s.multiscatter_recorded(false);
        CHECK(is(s, false, true));
        s.multiscatter_recorded(true);
        CHECK(is(s, false, true));
    }
    {
        LutState s = settled(); // handed out while no mode is set: nothing reads it
        s.multiscatter_exposed(false);
        CHECK(is(s, false, true));
        s.multiscatter_mode_changed(); // ... until a mode is set, which forces by itself
        CHECK(is(s, true, true));
    }
    {
        LutState s = settled(); // handed out with a mode set: writable texels, as the other two accessors
        s.multiscatter_exposed(true);
        CHECK(is(s, true, true));
        s.skyview_rows_recorded(0u, HEIGHT, HEIGHT);
        CHECK(is(s, false, true));
        // the pass that replaces texels the caller may have written changes what the sky-view LUT was computed from ...
        s.multiscatter_recorded(true);
        CHECK(is(s, true, true));
        s.skyview_rows_recorded(0u, HEIGHT, HEIGHT);
        s.multiscatter_recorded(true); // ... once: from then on the texels are the library's own again
        CHECK(is(s, false, true));
    }
    {
        LutState s = settled(); // a forced state stays forced through every new event
        s.skyview_exposed();
        s.multiscatter_recorded(true);
        s.multiscatter_exposed(false);
        CHECK(s.forceSkyview && s.multiscatterPresent);
    }
    printf("%s\n", failures == 0 ? "lut_state_multiscatter ok" : "lut_state_multiscatter FAILED");
    return failures == 0 ? 0 : 1;
}
