// lut_state.hpp — what the host knows about the two LUT blocks of a sky-view pipeline (szg_launch.hpp "transmittance LUT
// block", "sky-view LUT block", "LUT reuse"), as one state machine: a method per event, called by api_skyview.cpp and by
// nothing else. No HIP here, so that tests/cpp/lut_state.cpp walks the table on the CPU.
#pragma once

#include <cstdint>

namespace szg
{
struct LutState
{
    // false while the caller may have written the transmittance texels: the next consumer recomputes the block's status dword first
    bool tlutStatusValid = false;
    // the same for the sky-view LUT's status dword: false after a row-slice launch or after the texels were handed out
    bool slutStatusValid = false;
    // the status dword behind the sky-view LUT describes exactly the rows of the last slice launch, which were these
    bool sliceStatusKnown = false;
    uint32_t sliceRowBegin = 0, sliceRowEnd = 0;
    // the host knows the texels are stale: the reuse key (launch_lut_key) must not keep them
    bool forceTransmittance = true, forceSkyview = true;

    static bool whole(uint32_t rowBegin, uint32_t rowEnd, uint32_t height) { return rowBegin == 0u && rowEnd == height; }

    // reuse switched on or off: whatever was computed while it was off has no key on the device
    void reuse_switched() { forceTransmittance = forceSkyview = true; }
    // invalidated, or handed out through a view the caller may write through
    void transmittance_exposed()
    {
        tlutStatusValid = false;
        forceTransmittance = forceSkyview = true; // every sky-view texel is a function of the transmittance texels
    }
    void skyview_exposed()
    {
        slutStatusValid = sliceStatusKnown = false;
        forceSkyview = true;
    }
    void transmittance_recorded()
    {
        tlutStatusValid = true;
        forceTransmittance = false;
    }
    // a launch over all rows leaves the status dword right; a slice's dword knows its own rows only, and no key describes the
    // whole LUT afterwards
    void skyview_rows_recorded(uint32_t rowBegin, uint32_t rowEnd, uint32_t height)
    {
        bool const all = whole(rowBegin, rowEnd, height);
        slutStatusValid = all;
        sliceStatusKnown = forceSkyview = !all;
        sliceRowBegin = rowBegin;
        sliceRowEnd = rowEnd;
    }
    // Multi-scattering LUT (szg/multiscatter_sky.h). `multiscatterPresent`: the pipeline holds texels somebody wrote (the LUT
    // pass, or a caller through the accessor); a record call with a mode set is refused without them.
    bool multiscatterPresent = false;
    // the mode decides what every sky-view texel is: texels computed under another mode are stale
    void multiscatter_mode_changed() { forceSkyview = true; }
    // recorded by the library: the texels are a function of the atmosphere block and the transmittance LUT, both of which the
    // reuse key of the sky-view LUT covers (the block itself, and the transmittance LUT's generation): nothing to force
    // ... unless the texels it replaces were handed out before: those were a function of nothing the key knows
    void multiscatter_recorded(bool modeSet)
    {
        forceSkyview = forceSkyview || (modeSet && multiscatterHandedOut);
        multiscatterPresent = true;
        multiscatterHandedOut = false;
    }
    // handed out through a view the caller may write through; the sky-view LUT reads the texels only while a mode is set
    bool multiscatterHandedOut = false;
    void multiscatter_exposed(bool modeSet)
    {
        multiscatterPresent = multiscatterHandedOut = true;
        forceSkyview = forceSkyview || modeSet;
    }
    // all-gather of row slices: may rank `rank` of `nranks` stage the status dword as the status of its slice?
    bool slice_status_known(uint32_t rank, uint32_t nranks, uint32_t height) const
    {
        uint32_t const rows = height / nranks;
        return slutStatusValid || (sliceStatusKnown && sliceRowBegin == rank * rows && sliceRowEnd == (rank + 1u) * rows);
    }
    // `ok`: the stage, both exchanges and the reduce went through. No reuse key describes texels other ranks wrote.
    void rows_gathered(bool ok)
    {
        slutStatusValid = ok;
        sliceStatusKnown = false;
        forceSkyview = true;
    }
    // In front of a consumer: `rescan()` launches the re-scan of the texels and says whether the launch succeeded. It runs
    // only while the status is not known to be right, which it then is only if the launch succeeded.
    template <typename Rescan> void ensure_tlut_status(Rescan rescan) { tlutStatusValid = tlutStatusValid || rescan(); }
    template <typename Rescan> void ensure_slut_status(Rescan rescan) { slutStatusValid = slutStatusValid || rescan(); }
};
} // namespace szg
