// host_jpeg.cpp — the host half of include/szg/jpeg.h: marker parser and Huffman entropy decoder (baseline, extended
// sequential, progressive) into dequantised coefficient planes (rules 1 and 2), and the reconstruction in plain C++
// (rules 3-5, the functions of szg_jpeg_rules.hpp that the kernels compile too). CPU only, no HIP.
//
// Written from ITU-T T.81 (marker syntax annex B, Huffman procedures annexes C and F, progressive annex G); what the
// reference's decoder does where T.81 leaves a choice is stated in jpeg.h. Every read of the input goes through a bounds
// check; sizes are computed in size_t after the 32768 limit has been applied; every allocation may fail.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "szg/jpeg.h"
#include "szg_internal.hpp"
#include "szg_jpeg_rules.hpp"

struct szg_jpeg
{
    szg_jpeg_frame frame;
    int16_t* coefficients[3];
};

namespace szg
{
namespace
{
constexpr uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

uint32_t ceilDiv(uint32_t a, uint32_t b)
{
    return (a + b - 1u) / b;
}

struct Huffman
{
    bool defined = false;
    // codes of up to LOOK bits: (length << 8) | symbol, 0 = longer code
    static constexpr int LOOK = 9;
    uint16_t look[1 << LOOK];
    int32_t maxcode[18]; // first code of length l that is NOT used, left-aligned to 16 bits; [17] = sentinel
    int32_t delta[17];   // symbol index = (code >> (16 - l)) + delta[l]
    uint8_t symbols[256];
    int count = 0;

    // T.81 annex C. false: the lengths do not describe a prefix code
    bool build(const uint8_t counts[16], const uint8_t* values, int n)
    {
        defined = false;
        count = n;
        std::memcpy(symbols, values, (size_t)n);
        std::memset(look, 0, sizeof look);
        uint32_t code = 0;
        int k = 0;
        for (int l = 1; l <= 16; l++)
        {
            delta[l] = k - (int32_t)code;
            for (int i = 0; i < counts[l - 1]; i++, k++, code++)
            {
                if (l <= LOOK)
                {
                    uint32_t const first = code << (LOOK - l);
                    if (first + (1u << (LOOK - l)) > (1u << LOOK))
                    {
                        return false;
                    }
                    for (uint32_t f = 0; f < (1u << (LOOK - l)); f++)
                    {
                        look[first + f] = (uint16_t)((l << 8) | symbols[k]);
                    }
                }
            }
            if (code > (1u << l))
            {
                return false; // more codes of this length than the prefix leaves room for
            }
            maxcode[l] = (int32_t)(code << (16 - l));
            code <<= 1;
        }
        maxcode[17] = 0x7FFFFFFF;
        defined = true;
        return true;
    }
};

// The entropy-coded segment as a bit stream: FF 00 is a data byte FF, FF FF.. are fill bytes, FF xx stops the stream at
// the marker (`pos` stays on its FF) and zero bits follow. Running off the end of the input sets `exhausted`.
struct BitReader
{
    const uint8_t* data;
    size_t size, pos;
    uint32_t acc = 0; // the next bits, left-aligned
    int bits = 0;
    bool atMarker = false, exhausted = false;

    void fill()
    {
        while (bits <= 24)
        {
            uint32_t byte = 0;
            if (!atMarker && !exhausted)
            {
                if (pos >= size)
                {
                    exhausted = true;
                }
                else if (data[pos] != 0xFF)
                {
                    byte = data[pos++];
                }
                else
                {
                    size_t q = pos + 1;
                    while (q < size && data[q] == 0xFF)
                    {
                        q++; // fill bytes
                    }
                    if (q >= size)
                    {
                        exhausted = true;
                    }
                    else if (data[q] == 0x00 && q == pos + 1)
                    {
                        byte = 0xFF;
                        pos += 2;
                    }
                    else if (data[q] == 0x00)
                    {
                        // FF FF 00: fill bytes, then a stuffed FF
                        byte = 0xFF;
                        pos = q + 1;
                    }
                    else
                    {
                        pos = q - 1; // the FF in front of the marker code
                        atMarker = true;
                    }
                }
            }
            acc |= byte << (24 - bits);
            bits += 8;
        }
    }
    uint32_t peek(int n) // 1..16
    {
        if (bits < n)
        {
            fill();
        }
        return acc >> (32 - n);
    }
    void skip(int n)
    {
        acc <<= n;
        bits -= n;
    }
    uint32_t get(int n) // 0..16
    {
        if (n == 0)
        {
            return 0;
        }
        uint32_t const v = peek(n);
        skip(n);
        return v;
    }
    void reset()
    {
        acc = 0;
        bits = 0;
        atMarker = false;
    }
};

struct Component
{
    uint32_t id = 0, h = 1, v = 1, tq = 0;
    uint32_t width = 0, height = 0, blocksW = 0, blocksH = 0;
    int16_t* coef = nullptr;
    // per scan
    uint32_t td = 0, ta = 0;
    int32_t pred = 0;
};

struct Decoder
{
    Decoder(const uint8_t* bytes, size_t count) : data(bytes), size(count)
    {
        std::memset(quant, 0, sizeof quant);
    }

    const uint8_t* data;
    size_t size;
    size_t pos = 0;
    char error[200] = {0};
    int status = SZG_OK;

    uint16_t quant[4][64];
    bool quantDefined[4] = {false, false, false, false};
    Huffman dc[4], ac[4];
    uint32_t restartInterval = 0;
    bool haveFrame = false, progressive = false, jfif = false;
    int adobeTransform = -1;
    uint32_t width = 0, height = 0, hMax = 1, vMax = 1, mcusX = 0, mcusY = 0;
    uint32_t componentCount = 0;
    Component comp[3];
    uint32_t scans = 0;

    // scan state
    uint32_t scanCount = 0;
    uint32_t scanComp[3] = {0, 0, 0};
    uint32_t ss = 0, se = 63, ah = 0, al = 0;
    uint32_t eobrun = 0;

    bool fail(int code, const char* text)
    {
        if (status == SZG_OK)
        {
            status = code;
            std::snprintf(error, sizeof error, "szg_jpeg_open: %s", text);
        }
        return false;
    }
    bool parse(const char* text)
    {
        return fail(SZG_ERR_PARSE, text);
    }

    // ---- marker segments ----
    bool segment(size_t& begin, size_t& end) // the bytes after the length field
    {
        if (pos + 2 > size)
        {
            return parse("truncated: a marker segment has no length");
        }
        size_t const length = ((size_t)data[pos] << 8) | data[pos + 1];
        if (length < 2 || pos + length > size)
        {
            return parse("truncated: a marker segment's length runs past the end of the stream");
        }
        begin = pos + 2;
        end = pos + length;
        pos = end;
        return true;
    }

    bool readDQT()
    {
        size_t p, end;
        if (!segment(p, end))
        {
            return false;
        }
        while (p < end)
        {
            uint32_t const pq = data[p] >> 4, tq = data[p] & 15u;
            p++;
            if (pq > 1u || tq > 3u)
            {
                return parse("DQT: bad table precision or index");
            }
            size_t const need = pq ? 128 : 64;
            if (p + need > end)
            {
                return parse("DQT: table runs past its segment");
            }
            for (int i = 0; i < 64; i++)
            {
                quant[tq][ZIGZAG[i]] = pq ? (uint16_t)((data[p + 2 * i] << 8) | data[p + 2 * i + 1]) : data[p + i];
            }
            quantDefined[tq] = true;
            p += need;
        }
        return true;
    }

    bool readDHT()
    {
        size_t p, end;
        if (!segment(p, end))
        {
            return false;
        }
        while (p < end)
        {
            uint32_t const tc = data[p] >> 4, th = data[p] & 15u;
            p++;
            if (tc > 1u || th > 3u)
            {
                return parse("DHT: bad table class or index");
            }
            if (p + 16 > end)
            {
                return parse("DHT: table runs past its segment");
            }
            const uint8_t* const counts = data + p;
            int n = 0;
            for (int i = 0; i < 16; i++)
            {
                n += counts[i];
            }
            p += 16;
            if (n > 256 || p + (size_t)n > end)
            {
                return parse("DHT: more than 256 symbols, or the symbols run past the segment");
            }
            Huffman& table = tc ? ac[th] : dc[th];
            if (!table.build(counts, data + p, n))
            {
                return parse("DHT: the code lengths do not form a prefix code");
            }
            p += (size_t)n;
        }
        return true;
    }

    bool readDRI()
    {
        size_t p, end;
        if (!segment(p, end))
        {
            return false;
        }
        if (end - p != 2)
        {
            return parse("DRI: bad length");
        }
        restartInterval = ((uint32_t)data[p] << 8) | data[p + 1];
        return true;
    }

    bool readAPP(uint32_t marker)
    {
        size_t p, end;
        if (!segment(p, end))
        {
            return false;
        }
        if (marker == 0xE0 && end - p >= 5 && std::memcmp(data + p, "JFIF\0", 5) == 0)
        {
            jfif = true;
        }
        if (marker == 0xEE && end - p >= 12 && std::memcmp(data + p, "Adobe\0", 6) == 0)
        {
            adobeTransform = data[p + 11]; // tag 6, version 1, flags 2 + 2, transform
        }
        return true;
    }

    bool readSOF(uint32_t marker)
    {
        size_t p, end;
        if (!segment(p, end))
        {
            return false;
        }
        if (haveFrame)
        {
            return parse("more than one frame header");
        }
        if (end - p < 6)
        {
            return parse("SOF: bad length");
        }
        if (data[p] != 8)
        {
            return parse("only 8-bit precision is decoded (12-bit stream)");
        }
        height = ((uint32_t)data[p + 1] << 8) | data[p + 2];
        width = ((uint32_t)data[p + 3] << 8) | data[p + 4];
        componentCount = data[p + 5];
        if (width == 0u || height == 0u)
        {
            return parse("SOF: width or height is 0");
        }
        if (width > SZG_JPEG_MAX_EXTENT || height > SZG_JPEG_MAX_EXTENT)
        {
            return parse("width or height above 32768");
        }
        if (componentCount != 1u && componentCount != 3u)
        {
            return parse("only 1 or 3 components are decoded (2 components, or a 4-component CMYK / YCCK stream)");
        }
        if (end - p != 6 + 3 * (size_t)componentCount)
        {
            return parse("SOF: bad length");
        }
        hMax = vMax = 1;
        for (uint32_t c = 0; c < componentCount; c++)
        {
            Component& k = comp[c];
            k.id = data[p + 6 + 3 * c];
            k.h = data[p + 7 + 3 * c] >> 4;
            k.v = data[p + 7 + 3 * c] & 15u;
            k.tq = data[p + 8 + 3 * c];
            if (k.h < 1u || k.h > 4u || k.v < 1u || k.v > 4u)
            {
                return parse("SOF: sampling factor outside 1..4");
            }
            if (k.tq > 3u)
            {
                return parse("SOF: bad quantisation table index");
            }
            hMax = k.h > hMax ? k.h : hMax;
            vMax = k.v > vMax ? k.v : vMax;
        }
        for (uint32_t c = 0; c < componentCount; c++)
        {
            if (hMax % comp[c].h != 0u || vMax % comp[c].v != 0u)
            {
                return parse("SOF: a sampling factor does not divide the frame's maximum");
            }
        }
        mcusX = ceilDiv(width, 8u * hMax);
        mcusY = ceilDiv(height, 8u * vMax);
        size_t totalBlocks = 0;
        for (uint32_t c = 0; c < componentCount; c++)
        {
            Component& k = comp[c];
            k.width = ceilDiv(width * k.h, hMax);
            k.height = ceilDiv(height * k.v, vMax);
            k.blocksW = mcusX * k.h;
            k.blocksH = mcusY * k.v;
            totalBlocks += (size_t)k.blocksW * k.blocksH;
        }
        // every block costs a scan at least one bit: a frame with more blocks than the stream has bits cannot be complete,
        // and is refused before its planes are allocated
        if (totalBlocks / 8u > size)
        {
            return parse("truncated: the stream is shorter than one bit per block of its frame");
        }
        for (uint32_t c = 0; c < componentCount; c++)
        {
            Component& k = comp[c];
            k.coef = static_cast<int16_t*>(std::calloc((size_t)k.blocksW * k.blocksH * 64u, sizeof(int16_t)));
            if (k.coef == nullptr)
            {
                return fail(SZG_ERR_OUT_OF_MEMORY, "out of memory for the coefficient planes");
            }
        }
        progressive = marker == 0xC2;
        haveFrame = true;
        return true;
    }

    bool readSOS()
    {
        size_t p, end;
        if (!segment(p, end))
        {
            return false;
        }
        if (!haveFrame)
        {
            return parse("SOS before the frame header");
        }
        if (end - p < 1)
        {
            return parse("SOS: bad length");
        }
        scanCount = data[p];
        if (scanCount < 1u || scanCount > componentCount || end - p != 4 + 2 * (size_t)scanCount)
        {
            return parse("SOS: bad component count or length");
        }
        for (uint32_t i = 0; i < scanCount; i++)
        {
            uint32_t const id = data[p + 1 + 2 * i], tables = data[p + 2 + 2 * i];
            uint32_t which = componentCount;
            for (uint32_t c = 0; c < componentCount; c++)
            {
                if (comp[c].id == id)
                {
                    which = c;
                    break;
                }
            }
            if (which == componentCount)
            {
                return parse("SOS: unknown component id");
            }
            for (uint32_t before = 0; before < i; before++)
            {
                if (scanComp[before] == which)
                {
                    return parse("SOS: a component is named twice");
                }
            }
            if ((tables >> 4) > 3u || (tables & 15u) > 3u)
            {
                return parse("SOS: bad Huffman table index");
            }
            scanComp[i] = which;
            comp[which].td = tables >> 4;
            comp[which].ta = tables & 15u;
        }
        size_t const q = p + 1 + 2 * (size_t)scanCount;
        ss = data[q];
        se = data[q + 1];
        ah = data[q + 2] >> 4;
        al = data[q + 2] & 15u;
        if (progressive)
        {
            if (ss > 63u || se > 63u || ss > se || ah > 13u || al > 13u || (ss == 0u && se != 0u) || (ss != 0u && scanCount != 1u))
            {
                return parse("SOS: bad spectral selection or successive approximation");
            }
        }
        else
        {
            if (ss != 0u || ah != 0u || al != 0u)
            {
                return parse("SOS: spectral selection in a sequential stream");
            }
            se = 63;
        }
        for (uint32_t i = 0; i < scanCount; i++)
        {
            Component const& k = comp[scanComp[i]];
            bool const needDC = ss == 0u && ah == 0u, needAC = se > 0u;
            if ((needDC && !dc[k.td].defined) || (needAC && !ac[k.ta].defined))
            {
                return parse("SOS: a Huffman table the scan names was never defined");
            }
            if (!progressive && !quantDefined[k.tq])
            {
                return parse("SOS: a quantisation table the frame names was never defined");
            }
        }
        return true;
    }

    // ---- entropy decoding ----
    BitReader br{nullptr, 0, 0};

    int decodeSymbol(Huffman const& h) // -1: no such code
    {
        uint32_t const top = br.peek(16);
        uint16_t const fast = h.look[top >> (16 - Huffman::LOOK)];
        if (fast != 0)
        {
            br.skip(fast >> 8);
            return fast & 0xFF;
        }
        int l = Huffman::LOOK + 1;
        while (l <= 16 && (int32_t)top >= h.maxcode[l])
        {
            l++;
        }
        if (l > 16)
        {
            return -1;
        }
        int const index = (int)(top >> (16 - l)) + h.delta[l];
        if (index < 0 || index >= h.count)
        {
            return -1;
        }
        br.skip(l);
        return h.symbols[index];
    }

    // T.81 F.2.2.1 EXTEND of the next s bits, s = 0..15
    int32_t receiveExtend(int s)
    {
        if (s == 0)
        {
            return 0;
        }
        int32_t const v = (int32_t)br.get(s);
        return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    }

    static int16_t times(int32_t value, uint32_t q) // rule 2: the product truncated to int16
    {
        return (int16_t)(uint16_t)((uint32_t)value * q);
    }

    bool blockSequential(Component& k, int16_t* block)
    {
        const uint16_t* const q = quant[k.tq];
        int const t = decodeSymbol(dc[k.td]);
        if (t < 0 || t > 15)
        {
            return parse("bad Huffman code in a DC coefficient");
        }
        k.pred = (int32_t)((uint32_t)k.pred + (uint32_t)receiveExtend(t));
        std::memset(block, 0, 64 * sizeof(int16_t));
        block[0] = times(k.pred, q[0]);
        for (int i = 1; i < 64;)
        {
            int const rs = decodeSymbol(ac[k.ta]);
            if (rs < 0)
            {
                return parse("bad Huffman code in an AC coefficient");
            }
            int const r = rs >> 4, s = rs & 15;
            if (s == 0)
            {
                if (r != 15)
                {
                    break; // EOB
                }
                i += 16;
                continue;
            }
            i += r;
            if (i > 63)
            {
                return parse("an AC run leaves the block");
            }
            block[ZIGZAG[i]] = times(receiveExtend(s), q[ZIGZAG[i]]);
            i++;
        }
        return true;
    }

    bool blockProgressiveDC(Component& k, int16_t* block)
    {
        if (ah == 0u)
        {
            int const t = decodeSymbol(dc[k.td]);
            if (t < 0 || t > 15)
            {
                return parse("bad Huffman code in a DC coefficient");
            }
            k.pred = (int32_t)((uint32_t)k.pred + (uint32_t)receiveExtend(t));
            block[0] = (int16_t)(uint16_t)((uint32_t)k.pred << al);
        }
        else if (br.get(1) != 0u)
        {
            block[0] = (int16_t)(uint16_t)((uint32_t)(uint16_t)block[0] + (1u << al));
        }
        return true;
    }

    bool blockProgressiveAC(Component& k, int16_t* block)
    {
        Huffman const& h = ac[k.ta];
        if (ah == 0u)
        {
            if (eobrun > 0u)
            {
                eobrun--;
                return true;
            }
            for (uint32_t i = ss; i <= se;)
            {
                int const rs = decodeSymbol(h);
                if (rs < 0)
                {
                    return parse("bad Huffman code in an AC coefficient");
                }
                uint32_t const r = (uint32_t)rs >> 4, s = (uint32_t)rs & 15u;
                if (s == 0u)
                {
                    if (r < 15u)
                    {
                        eobrun = (1u << r) - 1u;
                        if (r > 0u)
                        {
                            eobrun += br.get((int)r);
                        }
                        break;
                    }
                    i += 16u;
                    continue;
                }
                i += r;
                if (i > se)
                {
                    return parse("an AC run leaves the spectral band");
                }
                block[ZIGZAG[i]] = (int16_t)(uint16_t)((uint32_t)receiveExtend((int)s) << al);
                i++;
            }
            return true;
        }
        // refinement, T.81 G.1.2.3
        uint32_t const plus = 1u << al;
        auto refine = [&](int16_t& c) {
            if (br.get(1) != 0u && ((uint32_t)(uint16_t)c & plus) == 0u)
            {
                c = (int16_t)(uint16_t)((uint32_t)(uint16_t)c + (c >= 0 ? plus : 0u - plus));
            }
        };
        uint32_t i = ss;
        if (eobrun == 0u)
        {
            while (i <= se)
            {
                int const rs = decodeSymbol(h);
                if (rs < 0)
                {
                    return parse("bad Huffman code in an AC coefficient");
                }
                uint32_t r = (uint32_t)rs >> 4;
                uint32_t const s = (uint32_t)rs & 15u;
                int16_t value = 0;
                if (s == 0u)
                {
                    if (r < 15u)
                    {
                        eobrun = (1u << r);
                        if (r > 0u)
                        {
                            eobrun += br.get((int)r);
                        }
                        break; // the rest of the band is refined below, as the first block of the run
                    }
                }
                else
                {
                    if (s != 1u)
                    {
                        return parse("a refinement scan carries a coefficient that is not +-1");
                    }
                    value = br.get(1) != 0u ? (int16_t)plus : (int16_t)(uint16_t)(0u - plus);
                }
                // skip r zero-history coefficients, refining the others on the way
                while (i <= se)
                {
                    int16_t& c = block[ZIGZAG[i]];
                    i++;
                    if (c != 0)
                    {
                        refine(c);
                    }
                    else
                    {
                        if (r == 0u)
                        {
                            if (value != 0)
                            {
                                c = value;
                            }
                            break;
                        }
                        r--;
                    }
                }
            }
        }
        if (eobrun > 0u)
        {
            for (; i <= se; i++)
            {
                int16_t& c = block[ZIGZAG[i]];
                if (c != 0)
                {
                    refine(c);
                }
            }
            eobrun--;
        }
        return true;
    }

    bool decodeBlock(Component& k, uint32_t bx, uint32_t by)
    {
        int16_t* const block = k.coef + ((size_t)by * k.blocksW + bx) * 64u;
        if (!progressive)
        {
            return blockSequential(k, block);
        }
        return ss == 0u ? blockProgressiveDC(k, block) : blockProgressiveAC(k, block);
    }

    // false: stop this scan (no restart marker where one belongs); the stream goes on at the next marker
    bool restart()
    {
        br.reset();
        size_t p = br.pos;
        while (p < size && data[p] == 0xFF && p + 1 < size && data[p + 1] == 0xFF)
        {
            p++;
        }
        if (p + 1 < size && data[p] == 0xFF && data[p + 1] >= 0xD0 && data[p + 1] <= 0xD7)
        {
            br.pos = p + 2;
            for (uint32_t c = 0; c < componentCount; c++)
            {
                comp[c].pred = 0;
            }
            eobrun = 0;
            return true;
        }
        return false;
    }

    bool readScan()
    {
        br = BitReader{data, size, pos};
        for (uint32_t c = 0; c < componentCount; c++)
        {
            comp[c].pred = 0;
        }
        eobrun = 0;
        uint32_t todo = restartInterval != 0u ? restartInterval : 0xFFFFFFFFu;
        bool stopped = false;
        if (scanCount == 1u)
        {
            Component& k = comp[scanComp[0]];
            uint32_t const w = ceilDiv(k.width, 8u), h = ceilDiv(k.height, 8u);
            for (uint32_t by = 0; by < h && !stopped; by++)
            {
                for (uint32_t bx = 0; bx < w; bx++)
                {
                    if (!decodeBlock(k, bx, by))
                    {
                        return false;
                    }
                    if (--todo == 0u)
                    {
                        todo = restartInterval;
                        if (!(by == h - 1u && bx == w - 1u) && !restart())
                        {
                            stopped = true;
                            break;
                        }
                    }
                }
            }
        }
        else
        {
            for (uint32_t my = 0; my < mcusY && !stopped; my++)
            {
                for (uint32_t mx = 0; mx < mcusX && !stopped; mx++)
                {
                    for (uint32_t i = 0; i < scanCount; i++)
                    {
                        Component& k = comp[scanComp[i]];
                        for (uint32_t y = 0; y < k.v; y++)
                        {
                            for (uint32_t x = 0; x < k.h; x++)
                            {
                                if (!decodeBlock(k, mx * k.h + x, my * k.v + y))
                                {
                                    return false;
                                }
                            }
                        }
                    }
                    if (--todo == 0u)
                    {
                        todo = restartInterval;
                        if (!(my == mcusY - 1u && mx == mcusX - 1u) && !restart())
                        {
                            stopped = true;
                        }
                    }
                }
            }
        }
        if (br.exhausted)
        {
            return parse("truncated: the stream ends inside a scan");
        }
        // on to the next marker: what is left of the entropy-coded segment is skipped
        pos = br.pos;
        while (pos + 1 < size && !(data[pos] == 0xFF && data[pos + 1] != 0x00 && data[pos + 1] != 0xFF && !(data[pos + 1] >= 0xD0 && data[pos + 1] <= 0xD7)))
        {
            pos++;
        }
        scans++;
        return true;
    }

    void dequantiseProgressive()
    {
        for (uint32_t c = 0; c < componentCount; c++)
        {
            Component& k = comp[c];
            const uint16_t* const q = quant[k.tq];
            size_t const n = (size_t)k.blocksW * k.blocksH * 64u;
            for (size_t i = 0; i < n; i++)
            {
                k.coef[i] = times(k.coef[i], q[i & 63u]);
            }
        }
    }

    bool run()
    {
        if (size < 4 || data[0] != 0xFF || data[1] != 0xD8)
        {
            return parse("not a JPEG stream (no SOI marker)");
        }
        pos = 2;
        for (;;)
        {
            if (pos + 2 > size)
            {
                return parse("truncated: the stream ends before its EOI marker");
            }
            if (data[pos] != 0xFF)
            {
                return parse("expected a marker");
            }
            uint32_t const marker = data[pos + 1];
            if (marker == 0xFF)
            {
                pos++; // fill byte
                continue;
            }
            pos += 2;
            bool ok = true;
            switch (marker)
            {
            case 0xD9: // EOI
                if (!haveFrame || scans == 0u)
                {
                    return parse("no frame or no scan before the EOI marker");
                }
                if (progressive)
                {
                    for (uint32_t c = 0; c < componentCount; c++)
                    {
                        if (!quantDefined[comp[c].tq])
                        {
                            return parse("a quantisation table the frame names was never defined");
                        }
                    }
                    dequantiseProgressive();
                }
                return true;
            case 0xC0:
            case 0xC1:
            case 0xC2:
                ok = readSOF(marker);
                break;
            case 0xC3:
            case 0xC7:
            case 0xCB:
            case 0xCF:
                return parse("lossless streams are not decoded");
            case 0xC5:
            case 0xC6:
            case 0xCD:
            case 0xCE:
                return parse("hierarchical streams are not decoded");
            case 0xC9:
            case 0xCA:
            case 0xCC:
                return parse("arithmetic-coded streams are not decoded");
            case 0xC4:
                ok = readDHT();
                break;
            case 0xDB:
                ok = readDQT();
                break;
            case 0xDD:
                ok = readDRI();
                break;
            case 0xDA:
                ok = readSOS() && readScan();
                break;
            case 0xD8:
                return parse("a second SOI marker");
            case 0x00:
            case 0x01:
            case 0xD0:
            case 0xD1:
            case 0xD2:
            case 0xD3:
            case 0xD4:
            case 0xD5:
            case 0xD6:
            case 0xD7:
                break; // stand-alone markers without a segment
            default:
                if (marker >= 0xE0 && marker <= 0xEF)
                {
                    ok = readAPP(marker);
                }
                else
                {
                    size_t b, e;
                    ok = segment(b, e); // COM, DNL and the reserved markers: skipped by their length
                }
                break;
            }
            if (!ok)
            {
                return false;
            }
        }
    }
};

// Why `f` is not a frame this library reconstructs (empty: it is one). Host and device entry points share it.
const char* frameProblem(const szg_jpeg_frame& f)
{
    if (f.plane_count != 1u && f.plane_count != 3u)
    {
        return "plane_count is not 1 or 3";
    }
    if ((f.plane_count == 1u) != (f.color == SZG_JPEG_GREY) || f.color > SZG_JPEG_RGB)
    {
        return "color does not fit plane_count";
    }
    if (f.width == 0u || f.height == 0u || f.width > SZG_JPEG_MAX_EXTENT || f.height > SZG_JPEG_MAX_EXTENT)
    {
        return "width or height outside 1..32768";
    }
    uint32_t hMax = 1, vMax = 1;
    for (uint32_t p = 0; p < f.plane_count; p++)
    {
        szg_jpeg_plane const& k = f.planes[p];
        if (k.h < 1u || k.h > 4u || k.v < 1u || k.v > 4u)
        {
            return "a sampling factor is outside 1..4";
        }
        hMax = k.h > hMax ? k.h : hMax;
        vMax = k.v > vMax ? k.v : vMax;
    }
    if (f.h_max != hMax || f.v_max != vMax)
    {
        return "h_max or v_max is not the maximum of the planes' factors";
    }
    uint32_t const mcusX = ceilDiv(f.width, 8u * hMax), mcusY = ceilDiv(f.height, 8u * vMax);
    for (uint32_t p = 0; p < f.plane_count; p++)
    {
        szg_jpeg_plane const& k = f.planes[p];
        if (hMax % k.h != 0u || vMax % k.v != 0u)
        {
            return "a sampling factor does not divide the maximum";
        }
        if (k.width != ceilDiv(f.width * k.h, hMax) || k.height != ceilDiv(f.height * k.v, vMax))
        {
            return "a plane's width or height does not follow from the frame's extent and its factors";
        }
        if (k.blocks_w != mcusX * k.h || k.blocks_h != mcusY * k.v)
        {
            return "a plane's blocks_w or blocks_h does not follow from the frame's extent and its factors";
        }
        if (k.coefficients == nullptr)
        {
            return "a plane's coefficients are NULL";
        }
    }
    return "";
}
} // namespace

const char* jpeg_frame_problem(const szg_jpeg_frame& frame)
{
    return frameProblem(frame);
}
} // namespace szg

int szg_jpeg_open(const void* bytes, size_t size, szg_jpeg** out)
{
    if (out != nullptr)
    {
        *out = nullptr;
    }
    if (bytes == nullptr || out == nullptr)
    {
        szg::set_last_error("szg_jpeg_open: NULL argument");
        return SZG_ERR_INVALID_ARGUMENT;
    }
    szg::Decoder* const d = new (std::nothrow) szg::Decoder(static_cast<const uint8_t*>(bytes), size);
    szg_jpeg* const jpeg = static_cast<szg_jpeg*>(std::calloc(1, sizeof(szg_jpeg)));
    if (d == nullptr || jpeg == nullptr)
    {
        delete d;
        std::free(jpeg);
        szg::set_last_error("szg_jpeg_open: out of memory");
        return SZG_ERR_OUT_OF_MEMORY;
    }
    bool const ok = d->run();
    if (!ok)
    {
        for (uint32_t c = 0; c < 3u; c++)
        {
            std::free(d->comp[c].coef);
        }
        szg::set_last_error(d->error);
        int const status = d->status;
        delete d;
        std::free(jpeg);
        return status;
    }
    szg_jpeg_frame& f = jpeg->frame;
    f.width = d->width;
    f.height = d->height;
    f.plane_count = d->componentCount;
    f.h_max = d->hMax;
    f.v_max = d->vMax;
    f.progressive = d->progressive ? 1u : 0u;
    bool const rgbIds = d->componentCount == 3u && d->comp[0].id == 'R' && d->comp[1].id == 'G' && d->comp[2].id == 'B';
    f.color = d->componentCount == 1u ? SZG_JPEG_GREY : ((rgbIds || (d->adobeTransform == 0 && !d->jfif)) ? SZG_JPEG_RGB : SZG_JPEG_YCBCR);
    for (uint32_t c = 0; c < d->componentCount; c++)
    {
        szg::Component const& k = d->comp[c];
        jpeg->coefficients[c] = k.coef;
        f.planes[c] = szg_jpeg_plane{k.coef, k.h, k.v, k.width, k.height, k.blocksW, k.blocksH};
    }
    delete d;
    *out = jpeg;
    return SZG_OK;
}

void szg_jpeg_destroy(szg_jpeg* jpeg)
{
    if (jpeg != nullptr)
    {
        for (int c = 0; c < 3; c++)
        {
            std::free(jpeg->coefficients[c]);
        }
        std::free(jpeg);
    }
}

int szg_jpeg_get_frame(const szg_jpeg* jpeg, szg_jpeg_frame* out)
{
    if (jpeg == nullptr || out == nullptr)
    {
        szg::set_last_error("szg_jpeg_get_frame: NULL argument");
        return SZG_ERR_INVALID_ARGUMENT;
    }
    *out = jpeg->frame;
    return SZG_OK;
}

int szg_jpeg_reconstruct_host(const szg_jpeg_frame* frame, uint32_t rgba_and, uint32_t rgba_or, uint8_t* rgba, size_t pitch_bytes)
{
    using namespace szg::jpeg;
    if (frame == nullptr || rgba == nullptr)
    {
        szg::set_last_error("szg_jpeg_reconstruct_host: NULL argument");
        return SZG_ERR_INVALID_ARGUMENT;
    }
    const char* const problem = szg::jpeg_frame_problem(*frame);
    if (problem[0] != '\0')
    {
        szg::set_last_error((std::string("szg_jpeg_reconstruct_host: ") + problem).c_str());
        return SZG_ERR_INVALID_ARGUMENT;
    }
    if (pitch_bytes < (size_t)frame->width * 4u)
    {
        szg::set_last_error("szg_jpeg_reconstruct_host: pitch_bytes is smaller than a row");
        return SZG_ERR_INVALID_ARGUMENT;
    }
    uint8_t* samples[3] = {nullptr, nullptr, nullptr};
    Plane planes[3];
    for (uint32_t p = 0; p < frame->plane_count; p++)
    {
        szg_jpeg_plane const& k = frame->planes[p];
        size_t const pitch = (size_t)k.blocks_w * 8u;
        samples[p] = static_cast<uint8_t*>(std::malloc(pitch * k.blocks_h * 8u));
        if (samples[p] == nullptr)
        {
            for (uint32_t q = 0; q < p; q++)
            {
                std::free(samples[q]);
            }
            szg::set_last_error("szg_jpeg_reconstruct_host: out of memory for the sample planes");
            return SZG_ERR_OUT_OF_MEMORY;
        }
        // rule 3: column pass, then row pass
        for (uint32_t by = 0; by < k.blocks_h; by++)
        {
            for (uint32_t bx = 0; bx < k.blocks_w; bx++)
            {
                const int16_t* const d = k.coefficients + ((size_t)by * k.blocks_w + bx) * 64u;
                uint32_t mid[64];
                for (int c = 0; c < 8; c++)
                {
                    uint32_t s[8], o[8];
                    for (int r = 0; r < 8; r++)
                    {
                        s[r] = (uint32_t)(int32_t)d[r * 8 + c];
                    }
                    idct1d(s, COLUMN_BIAS, o);
                    for (int r = 0; r < 8; r++)
                    {
                        mid[r * 8 + c] = (uint32_t)asr(o[r], COLUMN_SHIFT);
                    }
                }
                for (int r = 0; r < 8; r++)
                {
                    uint32_t o[8];
                    idct1d(mid + r * 8, ROW_BIAS, o);
                    uint8_t* const dst = samples[p] + ((size_t)by * 8u + (uint32_t)r) * pitch + (size_t)bx * 8u;
                    for (int c = 0; c < 8; c++)
                    {
                        dst[c] = (uint8_t)shiftClamp255(o[c], ROW_SHIFT);
                    }
                }
            }
        }
        planes[p] = Plane{samples[p], (uint32_t)pitch, frame->h_max / k.h, frame->v_max / k.v, k.height,
                          (frame->width + frame->h_max / k.h - 1u) / (frame->h_max / k.h)};
    }
    // rules 4 and 5
    for (uint32_t j = 0; j < frame->height; j++)
    {
        uint8_t* const row = rgba + (size_t)j * pitch_bytes;
        for (uint32_t x = 0; x < frame->width; x++)
        {
            uint32_t const c0 = upsampled(planes[0], x, j);
            uint32_t t;
            if (frame->plane_count == 1u)
            {
                t = texel(c0, c0, c0, false);
            }
            else
            {
                t = texel(c0, upsampled(planes[1], x, j), upsampled(planes[2], x, j), frame->color == SZG_JPEG_YCBCR);
            }
            t = (t & rgba_and) | rgba_or;
            row[4 * x + 0] = (uint8_t)t;
            row[4 * x + 1] = (uint8_t)(t >> 8);
            row[4 * x + 2] = (uint8_t)(t >> 16);
            row[4 * x + 3] = (uint8_t)(t >> 24);
        }
    }
    for (uint32_t p = 0; p < frame->plane_count; p++)
    {
        std::free(samples[p]);
    }
    return SZG_OK;
}
