// fuzz_jpeg.cpp — szg_jpeg_open / szg_jpeg_reconstruct_host over valid files and corrupted variants of them, as a stand-alone
// program built with -fsanitize=address,undefined over syzygy_amd/csrc/host_jpeg.cpp (tests/test_jpeg_sanitized.py): any
// out-of-bounds access, overflow or leak aborts it.
//
//   fuzz_jpeg N file...   every file as it is and N mutants of it. Prints "<inputs> inputs <decoded> decoded" and, per seed,
//                         "<file> <decoded mutants>"; exit 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "szg/jpeg.h"
#include "szg_internal.hpp"

namespace szg
{
static char g_error[256];
void set_last_error(const char* message)
{
    std::snprintf(g_error, sizeof g_error, "%s", message != nullptr ? message : "");
}
} // namespace szg

namespace
{
using Bytes = std::vector<uint8_t>;

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n)
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return n == 0 ? 0 : static_cast<uint32_t>((g_state >> 16) % n);
}

// offsets of the FF of every marker that carries a segment, up to the first SOS
std::vector<size_t> segments(const Bytes& d)
{
    std::vector<size_t> out;
    size_t at = 2;
    while (at + 4 <= d.size() && d[at] == 0xFF)
    {
        out.push_back(at);
        size_t const length = (size_t{d[at + 2]} << 8) | d[at + 3];
        if (d[at + 1] == 0xDA)
        {
            break;
        }
        at += 2 + length;
    }
    return out;
}

Bytes mutate(const Bytes& seed, uint32_t k)
{
    Bytes d = seed;
    std::vector<size_t> const seg = segments(seed);
    switch (k % 8)
    {
    case 0: // a few flipped bits anywhere
        for (uint32_t i = 0; i <= k % 3; i++)
        {
            d[rnd(static_cast<uint32_t>(d.size()))] ^= static_cast<uint8_t>(1u << rnd(8));
        }
        break;
    case 1: // truncation
        d.resize(rnd(static_cast<uint32_t>(d.size())));
        break;
    case 2: // a marker segment's length
        if (!seg.empty())
        {
            size_t const at = seg[rnd(static_cast<uint32_t>(seg.size()))];
            d[at + 2 + rnd(2)] ^= static_cast<uint8_t>(1u << rnd(8));
        }
        break;
    case 3: // Huffman tables: over-long codes and bad counts
        for (size_t at : seg)
        {
            if (d[at + 1] == 0xC4 && rnd(2) == 0)
            {
                d[at + 5 + rnd(16)] = static_cast<uint8_t>(rnd(256));
            }
        }
        break;
    case 4: // dimensions, component count and sampling factors
        for (size_t at : seg)
        {
            if (d[at + 1] >= 0xC0 && d[at + 1] <= 0xC2)
            {
                uint32_t const what = rnd(4);
                if (what == 0)
                {
                    d[at + 5] = static_cast<uint8_t>(rnd(256)); // height, high byte: up to 65535
                    d[at + 7] = static_cast<uint8_t>(rnd(256));
                }
                else if (what == 1)
                {
                    d[at + 5] = d[at + 7] = 0x80; // 32768+
                }
                else if (what == 2)
                {
                    d[at + 11 + 3 * rnd(3)] = static_cast<uint8_t>(rnd(256));
                }
                else
                {
                    d[at + 9] = static_cast<uint8_t>(rnd(6));
                }
            }
        }
        break;
    case 5: // restart markers out of order, dropped or doubled
        for (size_t i = seg.empty() ? 0 : seg.back(); i + 1 < d.size(); i++)
        {
            if (d[i] == 0xFF && d[i + 1] >= 0xD0 && d[i + 1] <= 0xD7 && rnd(3) == 0)
            {
                d[i + 1] = static_cast<uint8_t>(rnd(3) == 0 ? 0x00 : 0xD0 + rnd(8));
            }
        }
        d[rnd(static_cast<uint32_t>(d.size()))] ^= 1;
        break;
    case 6: // a byte of the scan header or the entropy-coded data
        if (!seg.empty())
        {
            size_t const from = seg.back();
            d[from + rnd(static_cast<uint32_t>(d.size() - from))] = static_cast<uint8_t>(rnd(256));
        }
        break;
    default: // a run of bytes overwritten
    {
        size_t const at = rnd(static_cast<uint32_t>(d.size()));
        for (size_t i = at; i < d.size() && i < at + 1 + rnd(8); i++)
        {
            d[i] = static_cast<uint8_t>(rnd(256));
        }
        break;
    }
    }
    return d;
}

bool decode(const Bytes& d)
{
    szg_jpeg* jpeg = nullptr;
    // the decoder gets an exact-size heap copy: one byte past the end is a sanitizer report
    uint8_t* const copy = static_cast<uint8_t*>(std::malloc(d.size() > 0 ? d.size() : 1));
    std::memcpy(copy, d.data(), d.size());
    int const status = szg_jpeg_open(copy, d.size(), &jpeg);
    std::free(copy);
    if (status != SZG_OK)
    {
        if (jpeg != nullptr || szg::g_error[0] == '\0')
        {
            std::fprintf(stderr, "a failed open left a handle or no text\n");
            std::exit(3);
        }
        return false;
    }
    szg_jpeg_frame frame;
    szg_jpeg_get_frame(jpeg, &frame);
    bool ok = false;
    if ((size_t)frame.width * frame.height <= (size_t{1} << 22))
    {
        Bytes rgba((size_t)frame.width * frame.height * 4u);
        ok = szg_jpeg_reconstruct_host(&frame, 0xFFFFFFFFu, 0u, rgba.data(), (size_t)frame.width * 4u) == SZG_OK;
    }
    szg_jpeg_destroy(jpeg);
    return ok;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 3)
    {
        std::fprintf(stderr, "usage: fuzz_jpeg N file...\n");
        return 2;
    }
    uint32_t const n = static_cast<uint32_t>(std::strtoul(argv[1], nullptr, 10));
    size_t inputs = 0, decoded = 0;
    std::vector<size_t> perSeed;
    for (int a = 2; a < argc; a++)
    {
        std::ifstream in(argv[a], std::ios::binary);
        Bytes const seed((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (seed.size() < 4)
        {
            std::fprintf(stderr, "cannot read %s\n", argv[a]);
            return 2;
        }
        inputs++;
        decoded += decode(seed) ? 1 : 0;
        size_t mutants = 0;
        for (uint32_t k = 0; k < n; k++)
        {
            inputs++;
            mutants += decode(mutate(seed, k)) ? 1 : 0;
        }
        decoded += mutants;
        perSeed.push_back(mutants);
    }
    std::printf("%zu inputs %zu decoded\n", inputs, decoded);
    for (int a = 2; a < argc; a++)
    {
        std::printf("%s %zu\n", argv[a], perSeed[(size_t)a - 2]);
    }
    return 0;
}
