// lut_state.cpp — host only, no HIP: the LUT bookkeeping of the sky-view pipeline (syzygy_amd/csrc/lut_state.hpp) walked
// event by event. tests/test_lut_state.py compiles this with g++ and runs it. T, S, K are tlutStatusValid, slutStatusValid and
// sliceStatusKnown; FT, FS the two force flags that make the reuse key recompute.
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

static bool is(const LutState& s, bool T, bool S, bool K, bool FT, bool FS)
{
    return s.tlutStatusValid == T && s.slutStatusValid == S && s.sliceStatusKnown == K && s.forceTransmittance == FT &&
           s.forceSkyview == FS;
}

constexpr uint32_t HEIGHT = 128u, RANKS = 4u; // rank r's slice: rows [32 r, 32 r + 32)

// everything valid, nothing forced: the state in which a later event's effect shows on every flag
static LutState settled()
{
    LutState s;
    s.transmittance_recorded();
    s.skyview_rows_recorded(0u, HEIGHT, HEIGHT);
    return s;
}

int main()
{
    // ---- every row of the table, from the initial state
    CHECK(is(LutState{}, false, false, false, true, true));
    {
        LutState s;
        s.reuse_switched();
        CHECK(is(s, false, false, false, true, true));
    }
    {
        LutState s;
        s.transmittance_exposed();
        CHECK(is(s, false, false, false, true, true));
    }
    {
        LutState s;
        s.skyview_exposed();
        CHECK(is(s, false, false, false, true, true));
    }
    {
        LutState s;
        s.transmittance_recorded();
        CHECK(is(s, true, false, false, false, true));
    }
    {
        LutState s; // whole: b = 0 and e = height
        CHECK(LutState::whole(0u, HEIGHT, HEIGHT) && !LutState::whole(0u, HEIGHT - 1u, HEIGHT) && !LutState::whole(1u, HEIGHT, HEIGHT));
        s.skyview_rows_recorded(0u, HEIGHT, HEIGHT);
        CHECK(is(s, false, true, false, true, false));
    }
    {
        LutState s;
        s.skyview_rows_recorded(32u, 64u, HEIGHT);
        CHECK(is(s, false, false, true, true, true));
        CHECK(s.sliceRowBegin == 32u && s.sliceRowEnd == 64u);
    }
    {
        LutState s;
        CHECK(!s.slice_status_known(0u, RANKS, HEIGHT));
        s.rows_gathered(true);
        CHECK(is(s, false, true, false, true, true));
        s.rows_gathered(false);
        CHECK(is(s, false, false, false, true, true));
    }
    {
        LutState s;
        int launches = 0;
        s.ensure_tlut_status([&] { launches++; return true; });
        s.ensure_slut_status([&] { launches++; return true; });
        CHECK(launches == 2 && is(s, true, true, false, true, true));
        s.ensure_tlut_status([&] { launches++; return true; });
        s.ensure_slut_status([&] { launches++; return true; });
        CHECK(launches == 2); // valid: no re-scan
    }
    // ---- the same events from the settled state, where each flag they touch is at the other value
    CHECK(is(settled(), true, true, false, false, false));
    {
        LutState s = settled();
        s.reuse_switched();
        CHECK(is(s, true, true, false, true, true));
    }
    {
        LutState s = settled();
        s.transmittance_exposed();
        CHECK(is(s, false, true, false, true, true));
    }
    {
        LutState s = settled();
        s.skyview_rows_recorded(0u, 32u, HEIGHT); // K set, so that the event has it to clear
        s.skyview_exposed();
        CHECK(is(s, true, false, false, false, true));
    }
    {
        LutState s = settled();
        s.skyview_rows_recorded(0u, 32u, HEIGHT);
        s.rows_gathered(true);
        CHECK(is(s, true, true, false, false, true));
    }
    // ---- sequence 1: a slice, then the gather as the rank that owns these rows: known
    {
        LutState s;
        s.skyview_rows_recorded(64u, 96u, HEIGHT);
        CHECK(s.slice_status_known(2u, RANKS, HEIGHT));
    }
    // ---- sequence 2: a slice, then the gather as another rank, or over another rank count: unknown
    {
        LutState s;
        s.skyview_rows_recorded(64u, 96u, HEIGHT);
        CHECK(!s.slice_status_known(1u, RANKS, HEIGHT) && !s.slice_status_known(3u, RANKS, HEIGHT));
        CHECK(!s.slice_status_known(1u, 2u, HEIGHT));
        LutState w = settled(); // a whole LUT is known to every rank
        CHECK(w.slice_status_known(1u, RANKS, HEIGHT));
    }
    // ---- sequence 3: whole, handed out, then ensure must launch
    {
        LutState s;
        s.skyview_rows_recorded(0u, HEIGHT, HEIGHT);
        int launches = 0;
        s.ensure_slut_status([&] { launches++; return true; });
        CHECK(launches == 0);
        s.skyview_exposed();
        s.ensure_slut_status([&] { launches++; return true; });
        CHECK(launches == 1 && s.slutStatusValid);
        s.transmittance_recorded();
        s.transmittance_exposed();
        s.ensure_tlut_status([&] { launches++; return true; });
        CHECK(launches == 2 && s.tlutStatusValid);
    }
    // ---- sequence 4: a failed ensure leaves the flag 0, and the next one launches again
    {
        LutState s;
        int launches = 0;
        s.ensure_tlut_status([&] { launches++; return false; });
        s.ensure_slut_status([&] { launches++; return false; });
        CHECK(launches == 2 && !s.tlutStatusValid && !s.slutStatusValid);
        s.ensure_tlut_status([&] { launches++; return true; });
        s.ensure_slut_status([&] { launches++; return true; });
        CHECK(launches == 4 && s.tlutStatusValid && s.slutStatusValid);
    }
    printf("%s\n", failures == 0 ? "lut_state ok" : "lut_state FAILED");
    return failures == 0 ? 0 : 1;
}
