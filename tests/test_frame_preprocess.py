"""CPU suite: raw frames -> network input (image_proc.preprocess_frames, csrc/dataprep.hip preprocess_frames_kernel).

The coefficient builder against a NumPy restatement of Pillow's BILINEAR arithmetic, and the kernel itself under the SIMT
emulator against live Pillow and the committed fixture (tests/golden/frame_preprocess.npz), bit for bit for the resized
uint8 frames and for the normalised fp32 network input."""
import numpy as np
import pytest
import torch
from PIL import Image

import make_frame_preprocess as mfp
from dream_amd import image_proc
from emu_util import emulated_hip

MEAN, STDEV = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def restated_coefficients(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter, vectorised over the outputs."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = 2 * int(np.ceil(support)) + 1
    c = (np.arange(n_out) + 0.5) * scale
    lo = np.maximum((c - support + 0.5).astype(np.int64), 0)
    hi = np.minimum((c + support + 0.5).astype(np.int64), n_in)
    n = hi - lo
    i = np.arange(ksize)[None, :]
    t = np.abs((i + lo[:, None] - c[:, None] + 0.5) * (1.0 / fs))
    w = np.where((t < 1.0) & (i < n[:, None]), 1.0 - t, 0.0)
    total = np.zeros(n_out)
    for j in range(ksize):                     # Pillow sums the taps in order
        total = total + w[:, j]
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    k = np.where(w < 0, np.trunc(w * (1 << 22) - 0.5), np.trunc(w * (1 << 22) + 0.5)).astype(np.int32)
    return np.stack([lo, n], axis=1).astype(np.int32), k


def two_pass_resize(frame, crop, out):
    """The integer two-pass resize of the restated coefficients: horizontal pass (rounded to uint8) over the rows the
    vertical pass reads, then the vertical pass (rounded to uint8)."""
    x0, y0, cw, ch = crop
    a = frame[y0:y0 + ch, x0:x0 + cw].astype(np.int64)
    hb, hk = restated_coefficients(cw, out[0])
    vb, vk = restated_coefficients(ch, out[1])

    def clip8(acc):
        return np.where(acc <= 0, 0, np.where(acc >= 255 << 22, 255, acc >> 22))
    mid = np.zeros((ch, out[0], 3), np.int64)
    r0, r1 = vb[0, 0], vb[-1, 0] + vb[-1, 1]
    for o, (lo, n) in enumerate(hb):
        mid[r0:r1, o] = clip8((1 << 21) + (a[r0:r1, lo:lo + n] * hk[o, :n][None, :, None]).sum(1))
    res = np.zeros((out[1], out[0], 3), np.int64)
    for o, (lo, n) in enumerate(vb):
        res[o] = clip8((1 << 21) + (mid[lo:lo + n] * vk[o, :n][:, None, None]).sum(0))
    return res.astype(np.uint8)


def host_input(u8_bhwc):
    """keypoints_from_image's ToTensor + Normalize (network.py:449-459 as dream_amd/network.py does it), per frame."""
    arr = u8_bhwc.astype(np.float32) / np.float32(255.0)
    x = (arr - np.asarray(MEAN, np.float32)) / np.asarray(STDEV, np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))


SIZE_PAIRS = [(480, 400), (400, 480), (1080, 400), (2160, 400), (720, 400), (13, 20), (40, 10), (16, 16), (100, 70),
              (24, 37), (1, 5), (5, 1), (1920, 711)]


@pytest.mark.parametrize("n_in,n_out", SIZE_PAIRS)
def test_coefficients_match_restatement(n_in, n_out):
    bounds, coeffs = image_proc.resample_coefficients(n_in, n_out)
    rb, rk = restated_coefficients(n_in, n_out)
    assert bounds.dtype == np.int32 and coeffs.dtype == np.int32
    assert np.array_equal(bounds, rb) and np.array_equal(coeffs, rk)
    assert (bounds[:, 0] >= 0).all() and (bounds.sum(1) <= n_in).all()
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()     # the kernel's tile windows rely on it


def test_restatement_matches_pillow():
    rs = np.random.RandomState(11)
    for (w, h), ref, mode in [((64, 48), (40, 40), "shrink-and-crop"), ((48, 64), (40, 40), "shrink-and-crop"),
                              ((37, 23), (50, 50), "resize"), ((90, 31), (20, 20), "shrink"), ((81, 61), (30, 30), "resize")]:
        f = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        crop, out = image_proc.preprocess_geometry((w, h), ref, mode)
        pil = np.asarray(image_proc.preprocess_image(Image.fromarray(f), ref, mode))
        assert np.array_equal(two_pass_resize(f, crop, out), pil), (w, h, mode)


def test_plan_geometry_and_tiles():
    plan = image_proc.preprocess_plan((640, 480), (400, 400), "shrink-and-crop")
    assert plan["crop"] == (80, 0, 480, 480) and plan["out"] == (400, 400)
    assert image_proc.preprocess_geometry((1920, 1080), (400, 400), "shrink") == ((0, 0, 1920, 1080), (711, 400))
    assert image_proc.preprocess_geometry((1280, 720), (400, 400), "resize") == ((0, 0, 1280, 720), (400, 400))
    # 4K into 400 x 400: ksize 13 and the LDS budget still met with fewer rows per tile
    plan = image_proc.preprocess_plan((3840, 2160), (400, 400), "shrink-and-crop")
    assert plan["vcoeffs"].shape[1] == 13 and plan["tile_rows"] < 32
    vb = plan["vbounds"]
    for y in range(0, 400, plan["tile_rows"]):
        last = min(y + plan["tile_rows"], 400) - 1
        assert vb[last, 0] + vb[last, 1] - vb[y, 0] <= plan["span_rows"]


def test_fixture_regenerates_byte_identical():
    import PIL
    with open(mfp.OUT, "rb") as f:
        committed = f.read()
    gold = np.load(mfp.OUT)
    written_by = str(gold["pillow_version"].item())
    if written_by != PIL.__version__:
        pytest.skip("fixture written by Pillow %s, %s installed" % (written_by, PIL.__version__))
    assert mfp.fixture_bytes() == committed


def test_fixture_matches_live_pillow():
    gold = np.load(mfp.OUT)
    for name, (_, _, _, ref, mode, _) in mfp.CASES.items():
        f = gold[name + ".frames"]
        assert np.array_equal(f, mfp.frames(name)), name
        assert np.array_equal(gold[name + ".pil"], mfp.pil_preprocess(f, ref, mode)), name


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """The SIMT-emulated library, built for this module into its own directory: a second pytest process running
    test_emulated_kernels.py at the same time rebuilds tests/emu/libdream_emu.so in place, and loading that file while
    another linker writes it is not safe."""
    import build_emu
    shared = build_emu.OUT
    build_emu.OUT = str(tmp_path_factory.mktemp("emu") / "libdream_emu.so")
    try:
        with emulated_hip() as lib:
            yield lib
    finally:
        build_emu.OUT = shared


@pytest.mark.parametrize("name", list(mfp.CASES))
def test_emulated_kernel_bit_exact(emu, name):
    gold = np.load(mfp.OUT)
    _, h, w, ref, mode, _ = mfp.CASES[name]
    frames = gold[name + ".frames"]
    pil = mfp.pil_preprocess(frames, ref, mode)
    assert np.array_equal(pil, gold[name + ".pil"]), name
    x, res, u8 = image_proc.preprocess_frames(torch.from_numpy(frames), ref, mode, MEAN, STDEV, return_u8=True)
    assert res == (pil.shape[2], pil.shape[1])
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == pil.shape
    assert np.array_equal(u8.numpy(), pil), name
    assert x.dtype == torch.float32 and torch.equal(x, host_input(pil)), name
    x2, res2 = image_proc.preprocess_frames(frames, ref, mode, MEAN, STDEV)          # numpy input, no uint8 output
    assert res2 == res and torch.equal(x2, x)


def test_emulated_kernel_batch_positions_and_views(emu):
    """Each frame of a batch is what it is alone, and a batch that starts at an unaligned offset of its storage is handled."""
    gold = np.load(mfp.OUT)
    _, _, _, ref, mode, _ = mfp.CASES["batch3"]
    frames = torch.from_numpy(gold["batch3.frames"])
    x, _ = image_proc.preprocess_frames(frames, ref, mode, MEAN, STDEV)
    for b in range(3):
        xb, _ = image_proc.preprocess_frames(frames[b:b + 1], ref, mode, MEAN, STDEV)
        assert torch.equal(xb[0], x[b])
    raw = torch.zeros(1 + frames.numel(), dtype=torch.uint8)
    raw[1:] = frames.reshape(-1)
    view = raw[1:].view(frames.shape)
    assert view.data_ptr() % 16 != 0
    xv, _ = image_proc.preprocess_frames(view, ref, mode, MEAN, STDEV)
    assert torch.equal(xv, x)


def test_emulated_none_is_the_plain_normalise(emu):
    frames = mfp.frames("batch3")
    x, res, u8 = image_proc.preprocess_frames(frames, (14, 14), "none", MEAN, STDEV, return_u8=True)
    assert res == (33, 25) and np.array_equal(u8.numpy(), frames)
    assert torch.equal(x, host_input(frames))

