"""Writes tests/golden/jpeg/*.jpg and tests/golden/jpeg/expected_rgba.npz: JPEG files written by Pillow (libjpeg) and what the
reference's decoder returns for a 4-channel request on each of them (include/szg/jpeg.h).

Needs Pillow, a C compiler and the reference tree; the test suite needs none of them. Usage:

    python tests/golden/make_jpeg_fixtures.py /path/to/reference

A small harness (its own main, the reference's stb_image.h included BY PATH) is written into a temporary directory and
compiled twice, default and -DSTBI_NO_SIMD; every file is decoded by both builds, the two must agree, and the result is
recorded. Nothing compiled and no text of the reference is kept.

Pillow's own decode of these files is NOT an expected value anywhere: its chroma upsampling differs from the reference's.
"""
import io
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "jpeg")

SIZES = [(1, 1), (2, 3), (7, 5), (8, 8), (9, 17), (17, 9), (33, 31), (130, 70)]
LAYOUTS = {"444": 0, "422": 1, "420": 2, "grey": None}
MODES = {"base": {}, "prog": {"progressive": True}, "rst": {"restart_marker_blocks": 1}}
# q92: most of the 64 table entries matter and blocks are dense; q12: blocks are mostly DC
QUALITIES = (92, 12)

HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#define STB_IMAGE_IMPLEMENTATION
#define STBI_ONLY_JPEG
#include STB_PATH
int main(int argc, char** argv)
{
    for (int i = 1; i + 1 < argc; i += 2)
    {
        int w = 0, h = 0, n = 0;
        unsigned char* p = stbi_load(argv[i], &w, &h, &n, 4);
        FILE* f = fopen(argv[i + 1], "wb");
        if (f == NULL) return 2;
        if (p == NULL) { w = h = 0; }
        fwrite(&w, 4, 1, f);
        fwrite(&h, 4, 1, f);
        if (p != NULL) fwrite(p, 4, (size_t)w * h, f);
        fclose(f);
        stbi_image_free(p);
    }
    return 0;
}
"""


def content(w, h, channels, seed):
    """left half a gradient, right half noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, channels), np.uint8)
    for c in range(channels):
        grad = ((x * (3 + c) + y * (5 - c)) * 255 // max(1, (w - 1) * (3 + c) + (h - 1) * (5 - c))).astype(np.uint8)
        noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
        img[..., c] = np.where(x < (w + 1) // 2, grad, noise)
    return img


def save(img, **options):
    buf = io.BytesIO()
    img.save(buf, "JPEG", **options)
    return bytearray(buf.getvalue())


def segments(data):
    """[(marker, offset of the FF, offset after the segment)] up to and including the first SOS header"""
    at, out = 2, []
    while at + 4 <= len(data):
        assert data[at] == 0xFF, at
        marker = data[at + 1]
        length = struct.unpack(">H", data[at + 2:at + 4])[0]
        out.append((marker, at, at + 2 + length))
        at += 2 + length
        if marker == 0xDA:
            break
    return out


def patch_sampling(data, component, value):
    for marker, at, _ in segments(data):
        if marker in (0xC0, 0xC1, 0xC2):
            data[at + 2 + 2 + 6 + 3 * component + 1] = value
            return data
    raise AssertionError("no SOF")


def patch_ids(data, ids):
    """component ids in SOF and in every SOS header"""
    at = 2
    while at + 4 <= len(data):
        if data[at] != 0xFF:
            at += 1
            continue
        marker = data[at + 1]
        if marker in (0x00, 0xFF) or 0xD0 <= marker <= 0xD9:
            at += 2
            continue
        length = struct.unpack(">H", data[at + 2:at + 4])[0]
        if marker in (0xC0, 0xC1, 0xC2):
            for c in range(3):
                data[at + 10 + 3 * c] = ids[data[at + 10 + 3 * c] - 1]
        if marker == 0xDA:
            for c in range(data[at + 4]):
                data[at + 5 + 2 * c] = ids[data[at + 5 + 2 * c] - 1]
        at += 2 + length
    return data


def adobe_transform0(data):
    """drop the JFIF APP0 segment, add an Adobe APP14 segment that says transform 0"""
    out = bytearray(data[:2])
    out += b"\xFF\xEE" + struct.pack(">H", 14) + b"Adobe\0" + bytes([100, 0, 0, 0, 0, 0])
    first = segments(data)
    for marker, at, end in first:
        if marker != 0xE0:
            out += data[at:end]
    out += data[first[-1][2]:]
    return out


def build_files():
    files = {}
    seed = 0
    for w, h in SIZES:
        for layout, subsampling in LAYOUTS.items():
            for q in QUALITIES:
                seed += 1  # the three entropy modes carry the same picture: the same coefficients in three codings
                for mode, options in MODES.items():
                    if subsampling is None:
                        img = Image.fromarray(content(w, h, 1, seed)[..., 0], "L")
                        data = save(img, quality=q, **options)
                    else:
                        img = Image.fromarray(content(w, h, 3, seed), "RGB")
                        data = save(img, quality=q, subsampling=subsampling, **options)
                    files[f"{layout}_{w}x{h}_{mode}_q{q}"] = data
    # further sampling layouts: the SOF sampling byte of the first component of a Pillow file, patched
    for n in (1, 9, 17, 24, 33):
        seed += 1
        data = save(Image.fromarray(content(n, n, 3, seed), "RGB"), quality=85, subsampling=1)
        files[f"h1v2_{n}x{n}_base_q85"] = patch_sampling(data, 0, 0x12)
    for w, h in ((32, 16), (31, 15), (33, 16)):
        seed += 1
        data = save(Image.fromarray(content(w, h, 3, seed), "RGB"), quality=85, subsampling=2)
        files[f"h4v1_{w}x{h}_base_q85"] = patch_sampling(data, 0, 0x41)
    for w, h in ((16, 32), (15, 31)):
        seed += 1
        data = save(Image.fromarray(content(w, h, 3, seed), "RGB"), quality=85, subsampling=2)
        files[f"h1v4_{w}x{h}_base_q85"] = patch_sampling(data, 0, 0x14)
    seed += 1
    base = save(Image.fromarray(content(17, 9, 3, seed), "RGB"), quality=85, subsampling=0)
    files["rgbids_17x9_base_q85"] = patch_ids(bytearray(base), b"RGB")
    files["adobe0_17x9_base_q85"] = adobe_transform0(bytearray(base))
    seed += 1
    cmyk = Image.fromarray(content(17, 9, 4, seed), "CMYK")
    files["refused_cmyk_17x9"] = save(cmyk, quality=85)
    return files


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    reference = sys.argv[1]
    stb = os.path.join(reference, "thirdparty", "stb", "include", "stb", "stb_image.h")
    assert os.path.exists(stb), stb
    os.makedirs(OUT, exist_ok=True)
    files = build_files()
    for name, data in files.items():
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(bytes(data))
    names = sorted(n for n in files if not n.startswith("refused_"))
    expected = {}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "harness.c")
        with open(src, "w") as f:
            f.write(HARNESS)
        results = []
        for tag, defines in (("simd", []), ("scalar", ["-DSTBI_NO_SIMD"])):
            exe = os.path.join(tmp, "harness_" + tag)
            subprocess.run(["gcc", "-O1", f'-DSTB_PATH="{stb}"', *defines, src, "-o", exe, "-lm"], check=True)
            args = []
            for n in names:
                args += [os.path.join(OUT, n + ".jpg"), os.path.join(tmp, f"{n}.{tag}")]
            subprocess.run([exe, *args], check=True)
            decoded = {}
            for n in names:
                raw = open(os.path.join(tmp, f"{n}.{tag}"), "rb").read()
                w, h = struct.unpack("<ii", raw[:8])
                assert w > 0 and h > 0, f"the reference refuses {n}"
                decoded[n] = np.frombuffer(raw[8:], np.uint8).reshape(h, w, 4).copy()
            results.append(decoded)
        for n in names:
            assert (results[0][n] == results[1][n]).all(), f"the reference's SIMD and scalar builds differ on {n}"
            # stored channel by channel, [4, h, w]: deflate then finds the constant alpha plane and a grey file's three equal
            # planes; tests/jpeg_fixtures.py puts them back together as [h, w, 4]
            planar = np.ascontiguousarray(results[1][n].transpose(2, 0, 1))
            # a progressive or restart-marker file whose picture the reference decodes exactly like its baseline sibling is
            # not stored again: tests/jpeg_fixtures.py falls back to the "_base_" key
            sibling = n.replace("_prog_", "_base_").replace("_rst_", "_base_")
            if sibling != n and sibling in expected and np.array_equal(expected[sibling], planar):
                continue
            expected[n] = planar
    np.savez_compressed(os.path.join(OUT, "expected_rgba.npz"), **expected)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"{len(files)} files, {len(expected)} expected images, {total} bytes in {OUT}")


if __name__ == "__main__":
    main()
