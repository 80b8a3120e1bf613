"""The numpy model of the PNG encoder (tests/png_ref.py) on its own: its files are valid PNG files of the input, read back
with Pillow and, independently, chunk by chunk with zlib and numpy; their sizes obey the header's statements.  No device."""
import io
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import png_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_png.h")
MODES = {1: "L", 3: "RGB", 4: "RGBA"}


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_files_decode_to_the_input(shape, level):
    from PIL import Image
    H, W, C = shape
    for name in R.CONTENTS:
        a, parts = R.case(name, shape, level)
        data = parts["file"]
        im = Image.open(io.BytesIO(data))
        assert im.mode == MODES[C] and im.size == (W, H), (name, im.mode, im.size)
        got = np.asarray(im)
        assert got.shape == a.shape and (got == a).all(), name
        # without a PNG library: chunks, CRCs, zlib.decompress of the joined IDAT data, filters undone in numpy
        assert (R.decode(data) == a).all(), name
        chunks = R.walk_chunks(data)
        assert [k for k, _ in chunks] == [b"IHDR"] + [b"IDAT"] * (R.segments_of(H * (1 + W * C)) + 1) + [b"IEND"], name
        assert len(data) <= R.bound(H, W, C), name
        if level == 0:
            assert len(data) == R.bound(H, W, C) and set(parts["types"].tolist()) == {0} and set(parts["forms"]) == {"stored"}
        else:
            assert len(data) <= len(R.case(name, shape, 0)[1]["file"]), name


def test_level_0_size_is_the_closed_formula():
    for H, W, C in R.SHAPES:
        total = H * (1 + W * C)
        want = 8 + 25 + 2 + -(-total // 32768) * 17 + total + 21 + 12
        assert R.bound(H, W, C) == want == len(R.case("noise", (H, W, C), 0)[1]["file"])


def test_noise_is_stored_and_constants_collapse():
    for shape in R.SHAPES:
        _, parts = R.case("noise", shape, 1)
        if shape[0] * shape[1] * shape[2] > 64:
            assert set(parts["forms"]) == {"stored"}, shape
    # a 258-byte match costs 13 bits under the fixed codes: 240 x 321 bytes are 3 chunks of about 128 such matches each
    a, parts = R.case("zeros", (240, 320, 1), 1)
    assert len(parts["file"]) * 50 < a.size, len(parts["file"])
    a, parts = R.case("ones", (240, 320, 1), 1)
    assert len(parts["file"]) * 50 < a.size, len(parts["file"])
    for shape in [(16, 4112, 3), (240, 320, 4)]:
        assert set(R.case("half", shape, 1)[1]["forms"]) == {"stored", "fixed"}, shape


def test_filter_choice_and_match_rule_on_small_streams():
    # costs (None, Sub, Up) of the rows: (40, 10, 40), (40, 10, 0), (46, 13, 6), (8, 8, 14): the least, and on a tie the lowest type
    a = np.array([[10, 10, 10, 10], [10, 10, 10, 10], [10, 11, 12, 13], [4, 0, 4, 0]], np.uint8)
    assert R.filter_types(a, 1).tolist() == [1, 2, 2, 0]
    assert R.filter_types(np.zeros((2, 3), np.uint8), 1).tolist() == [0, 0]
    # candidates 1, 2, 3, 4, L: the longest wins, ties to the earlier; nothing reaches in front of the segment
    seg = np.frombuffer(b"abcabcabcabcXXXXXXX", np.uint8)
    length, cand, dist = R.best_matches(seg, 12)
    assert length[3] == 9 and cand[3] == 2 and length[0] == 0 and length[13] == 6 and cand[13] == 0
    at, ln, cd, ds = R.parse(seg, 12)
    assert at.tolist() == [0, 1, 2, 3, 12, 13] and ln.tolist() == [0, 0, 0, 9, 0, 6]
    # the hash candidate: the least position of the bucket, any distance, lengths 4 .. 7, only where it beats the five
    seg = np.frombuffer(b"0123456789ABCDEFGHIJ23456789abcdefghij3456", np.uint8)
    length, cand, dist = R.best_matches(seg, 500)
    assert (length[20], cand[20], dist[20]) == (7, 5, 18) and (length[38], cand[38], dist[38]) == (4, 5, 35)
    assert length[21] == 7 and dist[21] == 18 and length[2] == 0 and length[39] == 0             # 39: three bytes are left
    at, ln, cd, ds = R.parse(seg, 500)
    assert at[20:].tolist() == [20, 27] + list(range(28, 38)) + [38] and ln[20:].tolist() == [7, 0] + [0] * 10 + [4]
    hl, hd = R.hash_candidate(np.frombuffer(b"XXXXXXXXXXXX", np.uint8))
    assert hl.tolist() == [0, 7, 7, 7, 7, 7, 6, 5, 4, 0, 0, 0] and hd[1:9].tolist() == list(range(1, 9))
    assert R.best_matches(np.frombuffer(b"XXXXXXXXXXXX", np.uint8), 500)[1].max() == 0          # ties stay with the five
    # the fixed form is what zlib reads: a raw deflate stream of it and a final empty block
    seg = np.frombuffer(b"abcabcabcabcXXXXXXX", np.uint8)
    body, nbytes, tokens = R.fixed_form(seg, 12)
    assert tokens == 6 and len(body) == nbytes
    assert zlib.decompress(body + b"\x01\x00\x00\xff\xff", wbits=-15) == seg.tobytes()


def fixtures(seed=5, H=240, W=320):
    """the three images whose sizes DESIGN.md section 10 quotes: a magma-mapped smooth field, a smooth RGB field with sigma = 2
    noise, a gray ramp"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    field = 0.5 + 0.25 * np.sin(x / 37.0 + rng.uniform(0, 6)) + 0.25 * np.cos(y / 23.0 + rng.uniform(0, 6))
    t = np.clip(field, 0, 1)[:, :, None]
    ramp4 = np.concatenate([255 * t, 255 * t ** 2, 255 * (1 - t) ** 0.5, np.full_like(t, 255)], axis=2)      # a smooth colour map
    smooth = np.stack([field, np.roll(field, 40, 1), np.roll(field, 40, 0)], axis=2) * 200 + rng.normal(0, 2, (H, W, 3))
    gray = np.broadcast_to((np.arange(W) * 255 // (W - 1))[None, :], (H, W))
    return {"magma": np.clip(ramp4, 0, 255).astype(np.uint8), "smooth_rgb": np.clip(smooth, 0, 255).astype(np.uint8),
            "gray_ramp": np.ascontiguousarray(gray).astype(np.uint8)}


@pytest.mark.parametrize("name", ["magma", "smooth_rgb", "gray_ramp"])
def test_fixture_sizes_beside_zlib(capsys, name):
    """The model's level-1 size beside ``len(zlib.compress(filtered, 1))`` of the same filtered stream; each must be smaller
    than the raw bytes.  Measured (240 x 320, seed 5):

        magma       raw 307200   level 1 144611   zlib 68497    ratio 2.11
        smooth_rgb  raw 230400   level 1 207502   zlib 128100   ratio 1.62
        gray_ramp   raw  76800   level 1    947   zlib   710    ratio 1.33

    With the five fixed distances alone ``smooth_rgb`` came out as its level-0 file, 230844 bytes: with sigma = 2 noise the
    filtered bytes are small numbers of either sign, a fixed-code literal costs 8 or 9 bits, and those distances find next to no
    match; the hash candidate finds the repeats that lie anywhere in the segment (zlib's own fixed-code strategy at its level
    9 reaches 167953 on that stream)."""
    a = fixtures()[name]
    parts = R.encode_parts(a, 1)
    ours, theirs = len(parts["file"]), len(zlib.compress(parts["stream"].tobytes(), 1))
    with capsys.disabled():
        print("\npng fixture %-10s raw %7d  model level 1 %7d  zlib.compress(filtered, 1) %7d  ratio %.2f"
              % (name, a.size, ours, theirs, ours / theirs))
    assert (R.decode(parts["file"]) == a).all()
    assert ours < a.size, (name, ours, a.size)


def test_header_is_plain_c_and_matches_the_tables(tmp_path):
    from gftorf_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gft_png_[a-z_0-9]+)\s*\(", src)))
    assert set(names) == set(_lib.PNG_EXPORTS), names
    assert "k_png.hip" in build.SOURCES
    prog = tmp_path / "png_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_png.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d %d\\n", (int)(sizeof(f) / sizeof(f[0])), (int)sizeof(gft_png_image)); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(prog), "-o",
                           str(tmp_path / "png_abi.o")])
    out = subprocess.check_output(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-include", "gftorf_png.h", "-x", "c",
                                   "-"], input="PNG_WORDS_ARE GFT_PNG_SEGMENT GFT_PNG_MAX_IMAGES GFT_PNG_CHUNK_SLOT GFT_PNG_HASH_BITS\n", text=True)
    consts = [int(x) for x in out.split("PNG_WORDS_ARE", 1)[1].split()]
    assert consts == [_lib.PNG_SEGMENT, _lib.PNG_MAX_IMAGES, _lib.PNG_CHUNK_SLOT, R.HASH_BITS] and consts[0] == R.SEGMENT
    assert consts[2] >= 12 + 2 + 5 + consts[0] and consts[2] % 16 == 0 and consts[1] >= 32
    import ctypes
    assert ctypes.sizeof(_lib.PngImage) == 40


def test_library_bound_is_the_models():
    import gftorf_amd
    from gftorf_amd import _lib, png
    assert gftorf_amd.png is png
    lib = _lib.load()
    for H, W, C in R.SHAPES + [(480, 640, 4), (1, 40000, 1)]:
        assert lib.gft_png_bound(H, W, C) == R.bound(H, W, C) == png.bound(H, W, C)
    for bad in [(0, 1, 1), (1, 0, 3), (4, 4, 2), (4, 4, 5)]:
        assert lib.gft_png_bound(*bad) == -1
        with pytest.raises(ValueError, match="gftorf_amd.png"):
            png.bound(*bad)
    total, offsets, sizes_at = png.layout(R.SHAPES)
    assert all(o % 16 == 0 for o in offsets) and sizes_at % 16 == 0 and total == sizes_at + 8 * len(R.SHAPES)
    assert all(b - a >= R.bound(*s) for a, b, s in zip(offsets, offsets[1:] + [sizes_at], R.SHAPES))
    segs = sum(R.segments_of(H * (1 + W * C)) for H, W, C in R.SHAPES)
    assert png.scratch_bytes(R.SHAPES) >= segs * _lib.PNG_CHUNK_SLOT + sum(s[0] for s in R.SHAPES)
