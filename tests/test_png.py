"""gftorf_amd.png on the device: the files equal the numpy model's (tests/png_ref.py) byte for byte, sizes included, at both
levels, and Pillow decodes them to the input."""
import io

import numpy as np
import pytest
import torch

import png_ref as R

MODES = {1: "L", 3: "RGB", 4: "RGBA"}


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(data))))


def expanded(images):
    """{name: numpy image} with every [4, H, W] quad as its four planes name0 .. name3, as png.encode names them"""
    out = {}
    for k, a in images.items():
        if a.ndim == 3 and a.shape[0] == 4 and a.shape[2] not in (3, 4):
            out.update({"%s%d" % (k, q): a[q] for q in range(4)})
        else:
            out[k] = a
    return out


def check_files(files, images, level, what):
    """every file of {name: bytes-like} against the model's file of the numpy image of that name, and through Pillow"""
    assert list(files) == list(images), (what, list(files))
    for name, a in images.items():
        got, want = bytes(files[name]), R.encode(a, level)
        assert len(got) == len(want), (what, name, len(got), len(want))
        assert got == want, (what, name, next(k for k in range(len(want)) if got[k] != want[k]))
        back = pillow(got)
        assert back.shape == a.shape and (back == a).all(), (what, name)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("name", R.CONTENTS)
def test_device_files_are_the_models(name, level, gpu):
    """every shape of the list with one content in one call; the call repeated gives the same bytes"""
    from gftorf_amd import png
    host = {"%dx%dx%d" % s: R.case(name, s, level)[0] for s in R.SHAPES}
    images = {k: torch.tensor(a, device=gpu) for k, a in host.items()}
    batch = png.encode(images, level=level)
    assert batch.names == list(host) and batch.sizes.dtype == torch.int64 and batch.sizes.device == gpu
    assert batch.offsets == png.layout(R.SHAPES)[1]
    files = batch.to_host()
    sizes = batch.sizes.cpu().tolist()
    for k, s in zip(host, R.SHAPES):
        want = R.case(name, s, level)[1]["file"]
        assert sizes[list(host).index(k)] == len(want) == len(files[k]), (k, len(want))
        assert files[k] == want, (k, next(i for i in range(len(want)) if files[k][i] != want[i]))
        back = pillow(files[k])
        assert back.shape == host[k].shape and (back == host[k]).all(), k
    again = png.encode(images, level=level).to_host()
    assert again == files
    for k, a in host.items():
        assert np.array_equal(images[k].cpu().numpy(), a), k                       # the sources are untouched


def debug_inputs(gpu, H, W, seed=3):
    import test_present_debug as TD
    v, _ = TD.draw_debug(np.random.default_rng(seed), H, W, (2, 0, 3, 1), 1, "plain")
    return TD.kwargs_on(gpu, v)


@pytest.mark.gpu
def test_a_debug_sheet_in_one_call(gpu):
    """the 19 images of a debug sheet, gray, RGB and RGBA, read where they lie in the sheet"""
    from gftorf_amd import present, png
    sheet = present.debug_images(**debug_inputs(gpu, 36, 52))
    assert len(sheet) == 19 and sum(t.dim() == 3 and t.shape[0] == 4 for t in sheet.values()) == 3           # three of them quads
    base = min(t.data_ptr() for t in sheet.values())
    assert all(t.data_ptr() >= base and t.dtype == torch.uint8 for t in sheet.values())
    for level in (1, 0):
        files = png.encode(sheet, level=level).to_host()
        want = expanded({k: t.cpu().numpy() for k, t in sheet.items()})
        assert len(want) == 28 and {a.shape[2] if a.ndim == 3 else 1 for a in want.values()} == {1, 3, 4}
        check_files(files, want, level, "debug sheet level %d" % level)


@pytest.mark.gpu
def test_row_strides_and_quads(gpu):
    """images cut out of wider ones (a row stride, odd source addresses) and a [4, H, W] quad as four gray files"""
    from gftorf_amd import png
    rng = np.random.default_rng(11)
    wide = np.repeat(rng.integers(0, 256, (45, 50, 3), dtype=np.uint8), 4, axis=1)            # [45, 200, 3], runs of 4 pixels
    gray = np.repeat(rng.integers(0, 256, (70, 90), dtype=np.uint8), 7, axis=1)               # [70, 630]
    quad = (np.arange(4 * 33 * 129).reshape(4, 33, 129) // 5 % 251).astype(np.uint8)
    dw, dg, dq = (torch.tensor(a, device=gpu) for a in (wide, gray, quad))
    images = {"cut": dw[3:40, 7:188], "gray": dg[:, 1:602], "row": dg[5:6, 3:], "quad": dq, "rgba": dq.permute(1, 2, 0)[:, :, :4].contiguous()}
    want = {"cut": wide[3:40, 7:188], "gray": gray[:, 1:602], "row": gray[5:6, 3:], "quad0": quad[0], "quad1": quad[1], "quad2": quad[2],
            "quad3": quad[3], "rgba": np.ascontiguousarray(quad.transpose(1, 2, 0))}
    assert not images["cut"].is_contiguous() and images["gray"].data_ptr() % 2 == 1
    files = png.encode(images).to_host()
    check_files(files, want, 1, "strided")
    # a quad cut out of a sheet keeps its planes' strides
    files = png.encode({"q": dq[:, 2:31, 3:100]}, level=1).to_host()
    check_files(files, {"q%d" % k: quad[k, 2:31, 3:100] for k in range(4)}, 1, "quad view")


@pytest.mark.gpu
def test_a_captured_graph_follows_the_contents(gpu):
    """one capture replayed over changed image contents: sizes and bytes follow each replay (no size is baked in on the host,
    nothing relies on a cleared buffer)"""
    from gftorf_amd import png
    shapes = [(40, 300, 3), (33, 1023, 1), (9, 17, 4)]
    first = {"%d" % k: R.content("half", s, seed=1) for k, s in enumerate(shapes)}
    second = {"%d" % k: R.content(c, s, seed=2) for k, (s, c) in enumerate(zip(shapes, ("ramp", "noise", "zeros")))}
    third = {"%d" % k: R.content(c, s, seed=3) for k, (s, c) in enumerate(zip(shapes, ("noise", "ones", "period3")))}
    images = {k: torch.tensor(a, device=gpu) for k, a in first.items()}
    total = png.layout(shapes)[0]
    out = torch.zeros((total,), device=gpu, dtype=torch.uint8)
    scratch = torch.zeros((png.scratch_bytes(shapes),), device=gpu, dtype=torch.uint8)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = png.encode(images, out=out, scratch=scratch)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    check_files(eager.to_host(), first, 1, "eager")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = png.encode(images, out=out, scratch=scratch)
    for what, contents in (("second", second), ("third", third), ("first", first)):
        for k, a in contents.items():
            images[k].copy_(torch.tensor(a, device=gpu))
        out.fill_(0xa5)
        scratch.fill_(0x5a)
        graph.replay()
        torch.cuda.synchronize()
        check_files(captured.to_host(), contents, 1, "replayed " + what)


@pytest.mark.gpu
def test_png_sheets(gpu):
    """two tags through two slots, a third submit raises, ready(wait=True) yields both in order; every file decodes to what
    ViewSheets yields for the same inputs, the float depths come through bit-equal"""
    import test_present as TP
    from gftorf_amd import present, png
    vkw = TP.kwargs_on(gpu, TP.make_view(21, 37))
    dkw = debug_inputs(gpu, 18, 26, seed=4)
    flow, gt_flow = torch.randn(3, 9, 11, device=gpu), torch.randn(2, 9, 11, device=gpu)
    plain = present.ViewSheets(slots=2)
    plain.submit("view", **vkw)
    plain.submit_debug("debug", **dkw)
    want = {tag: {k: a.copy() for k, a in images.items()} for tag, images in plain.ready(wait=True)}
    plain.submit_flow("flow", flow, gt_flow)
    want.update({tag: {k: a.copy() for k, a in images.items()} for tag, images in plain.ready(wait=True)})
    sheets = png.PngSheets(slots=2)
    sheets.submit_view("view", **vkw)
    sheets.submit_debug("debug", **dkw)
    with pytest.raises(RuntimeError, match="all 2 slots"):
        sheets.submit_flow("flow", flow, gt_flow)
    got = {}
    for tag, files in sheets.ready(wait=True):
        got[tag] = {k: (v.copy() if isinstance(v, np.ndarray) else bytes(v)) for k, v in files.items()}
    sheets.submit_flow("flow", flow, gt_flow)                                      # both slots are free again
    sheets.submit("own", {"a": torch.full((5, 6), 9, device=gpu, dtype=torch.uint8), "f": torch.arange(6.0, device=gpu).view(2, 3)})
    for tag, files in sheets.ready(wait=True):
        got[tag] = {k: (v.copy() if isinstance(v, np.ndarray) else bytes(v)) for k, v in files.items()}
    assert list(got) == ["view", "debug", "flow", "own"]
    assert {"depth_tof_f", "depth_norm_f", "quad"} <= set(want["view"])
    for tag in ("view", "debug", "flow"):
        names = []
        for k, a in want[tag].items():
            if a.dtype != np.uint8:
                assert got[tag][k].dtype == a.dtype and np.array_equal(got[tag][k].view(np.uint32), a.view(np.uint32)), (tag, k)
                names.append(k)
            elif a.ndim == 3 and a.shape[0] == 4 and a.shape[2] not in (3, 4):
                for q in range(4):
                    assert np.array_equal(pillow(got[tag]["%s%d" % (k, q)]), a[q]), (tag, k, q)
                    assert got[tag]["%s%d" % (k, q)] == R.encode(a[q], 1), (tag, k, q)
                names += ["%s%d" % (k, q) for q in range(4)]
            else:
                assert np.array_equal(pillow(got[tag][k]), a), (tag, k)
                assert got[tag][k] == R.encode(a, 1), (tag, k)
                names.append(k)
        assert sorted(got[tag]) == sorted(names), tag
    assert np.array_equal(pillow(got["own"]["a"]), np.full((5, 6), 9, np.uint8)) and got["own"]["f"].tolist() == [[0, 1, 2], [3, 4, 5]]


@pytest.mark.gpu
def test_save_writes_the_files(gpu, tmp_path):
    from gftorf_amd import png
    a = R.content("ramp", (12, 31, 3))
    files = png.encode({"ramp": torch.tensor(a, device=gpu)}).to_host()
    files["depth"] = np.arange(6, dtype=np.float32).reshape(2, 3)
    png.save(files, lambda name: str(tmp_path / (name + (".npy" if name == "depth" else ".png"))))
    assert (tmp_path / "ramp.png").read_bytes() == R.encode(a, 1)
    assert np.array_equal(np.load(tmp_path / "depth.npy"), files["depth"])


@pytest.mark.gpu
def test_errors_are_raised_before_any_launch(gpu, monkeypatch):
    from gftorf_amd import _lib, png
    lib = _lib.load()
    good = torch.zeros((6, 7, 3), device=gpu, dtype=torch.uint8)

    class NoLaunch:
        def __getattr__(self, name):
            if name == "gft_png_encode":
                raise AssertionError("gft_png_encode was reached")
            return getattr(lib, name)
    monkeypatch.setattr(_lib, "load", lambda: NoLaunch())
    small = torch.zeros((png.layout([(6, 7, 3)])[0] - 1,), device=gpu, dtype=torch.uint8)
    for images, kw, error, text in [
            ({"a": good.float()}, {}, TypeError, "a must be torch.uint8"),
            ({"a": torch.zeros((6, 7, 2), device=gpu, dtype=torch.uint8)}, {}, RuntimeError, r"\[H, W, 3\]"),
            ({"a": torch.zeros((6, 7, 5), device=gpu, dtype=torch.uint8)}, {}, RuntimeError, r"\[H, W, 3\]"),
            ({"a": good.cpu()}, {}, RuntimeError, "no CPU path"),
            ({"a": good}, {"out": small}, ValueError, "out must be"),
            ({"a": good}, {"out": small.cpu()}, RuntimeError, "no CPU path"),
            ({"a": good}, {"scratch": small[:16]}, ValueError, "scratch must be"),
            ({"a": good}, {"level": 2}, ValueError, "level must be 0 or 1"),
            ({"a": good.permute(1, 0, 2)}, {}, RuntimeError, "strides"),
            ({"a": good[:, :, 0]}, {}, RuntimeError, "strides"),
            ({}, {}, ValueError, "non-empty dict"),
            ({"q": torch.zeros((4, 5, 6), device=gpu, dtype=torch.uint8), "q1": good[:, :, :1].contiguous()[:, :, 0]}, {}, ValueError, "named alike"),
            ({"i%d" % k: good for k in range(png.MAX_IMAGES + 1)}, {}, ValueError, "at most")]:
        with pytest.raises(error, match=text):
            png.encode(images, **kw)
    monkeypatch.undo()
    # the C entry point checks on its own what the wrapper cannot get wrong
    table = (_lib.PngImage * 1)()
    table[0].src, table[0].row_stride, table[0].out_offset, table[0].H, table[0].W, table[0].channels = good.data_ptr(), 21, 0, 6, 7, 3
    out = torch.zeros((png.layout([(6, 7, 3)])[0],), device=gpu, dtype=torch.uint8)
    scratch = torch.zeros((png.scratch_bytes([(6, 7, 3)]),), device=gpu, dtype=torch.uint8)
    sizes = torch.zeros((1,), device=gpu, dtype=torch.int64)
    call = lambda **o: lib.gft_png_encode(None, o.get("count", 1), table, o.get("level", 1), out.data_ptr(), o.get("out_bytes", out.numel() - 8),
                                          sizes.data_ptr(), scratch.data_ptr() + o.get("shift", 0), o.get("scratch_bytes", scratch.numel()))
    for o, text in [(dict(count=0), "images"), (dict(level=3), "level"), (dict(out_bytes=100), "out holds"), (dict(scratch_bytes=64), "scratch holds"),
                    (dict(shift=4), "16-byte aligned")]:
        assert call(**o) != 0 and text in _lib.last_error(), (o, _lib.last_error())
    torch.cuda.synchronize()
    assert int(sizes.item()) == 0 and int(out.sum().item()) == 0
