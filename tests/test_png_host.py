"""The segment coder of the PNG encoder (csrc/gft_png_coder.h: the very functions k_png_segment calls between its barriers)
compiled for the host with the address and undefined-behaviour sanitizers (tests/png_host.cpp) and run thread by thread: every
chunk and every Adler part equals the numpy model's, and no step reads or writes outside the workgroup's LDS or the image.
No device."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import png_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path_factory.mktemp("png_host") / "png_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gftorf_amd", "csrc"),
                           os.path.join(ROOT, "tests", "png_host.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_coder_equals_the_model(program, tmp_path, shape):
    H, W, C = shape
    cases, args = [], []
    for name in R.CONTENTS:
        for level in (0, 1):
            a, parts = R.case(name, shape, level)
            src, dst = tmp_path / ("%s_%d.in" % (name, level)), tmp_path / ("%s_%d.out" % (name, level))
            src.write_bytes(struct.pack("<4i", H, W, C, level) + parts["types"].tobytes() + a.tobytes())
            cases.append((name, level, parts, dst))
            args += [str(src), str(dst)]
    r = subprocess.run([program] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    for name, level, parts, dst in cases:
        data, at = dst.read_bytes(), 0
        for s, want in enumerate(parts["chunks"]):
            n, A, B = struct.unpack("<3I", data[at:at + 12])
            got = data[at + 12:at + 12 + n]
            at += 12 + n
            seg = parts["stream"][s * R.SEGMENT:(s + 1) * R.SEGMENT].astype(np.int64)
            assert got == want, (name, level, s, n, len(want))
            assert (A, B) == (int(seg.sum() % 65521), int(((len(seg) - np.arange(len(seg))) * seg).sum() % 65521)), (name, level, s)
        assert at == len(data)
