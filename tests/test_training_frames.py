"""CPU suite: training batches from raw frames (image_proc.training_batch_from_frames; csrc/dataprep.hip
training_keypoints_kernel, augment_noise_kernel, augment_mean_kernel, augment_warp_kernel under the SIMT emulator).

The keypoint chain and the belief maps against the committed outputs of the reference's own functions
(tests/golden/training_frames.npz), the image against preprocess_frames / live Pillow, and the augmentation against the NumPy
restatement below of this package's definition.  Every comparison is bit for bit.

The definition restated (u = resized uint8 net-input frame [h,w,3], one table row per frame):
  1. noise: n = clip(rint(fp32(u) + sigma * z)), fp32, half to even; z = Q[mix(seed, i) >> 20] with i the linear index of pixel
     and channel, mix = murmur3's 32-bit finaliser of seed + i * 0x9E3779B9, Q = fp32 of the standard-normal quantiles at
     (j + 0.5) / 4096 (float64); sigma = 0 leaves u.
  2. brightness / contrast: m = fp32(sum(n) / count in float64); c = clip(rint(alpha * n + beta * m)), each product and the sum
     rounded on their own in fp32.
  3. shift-scale-rotate: source position s = Minv (x, y) in float64 (products and sums rounded one by one, left to right),
     fixed = floor(s * 32 + 0.5) (kept within +-2^40), integer part and 5 fraction bits, taps by reflect-101, value
     (sum(w * c(tap)) + 512) >> 10 with weights (32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx*fy.
  4. ((fp32(v) / 255) - mean) / stdev in fp32, NCHW.
Keypoints: k' = M k in float64 (skipped for an identity row), then net input -> net output -> float32."""
from statistics import NormalDist

import numpy as np
import pytest
import torch

import make_frame_preprocess as mfp
import make_training_frames as mtf
from dream_amd import image_proc
from emu_util import emulated_hip
from ref_import import have_reference
from test_frame_preprocess import MEAN, STDEV, host_input

QUANTILES = np.array([NormalDist().inv_cdf((j + 0.5) / 4096) for j in range(4096)]).astype(np.float32)


# ---- the NumPy restatement ------------------------------------------------------------------------------------------
def mix(seed, idx):
    h = (np.uint64(seed) + idx.astype(np.uint64) * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h


def round_clip(v):
    assert v.dtype == np.float32
    v = np.rint(v)
    return np.where(~(v > 0), 0, np.where(v >= 255, 255, v)).astype(np.int64)


def restated_noise(u, sigma, seed):
    if np.float32(sigma) == 0:
        return u.astype(np.int64)
    z = QUANTILES[(mix(seed, np.arange(u.size)) >> np.uint64(20)).astype(np.int64)].reshape(u.shape)
    return round_clip(u.astype(np.float32) + np.float32(sigma) * z)


def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    r = np.mod(i, p)
    return np.where(r < n, r, p - r)


def restated_augment(u, sigma, seed, alpha, beta, inverse):
    """-> augmented uint8 frame [h,w,3] of one resized frame u for one table row."""
    h, w, _ = u.shape
    n = restated_noise(u, sigma, seed)
    m = np.float32(np.float64(int(n.sum())) / np.float64(n.size))
    bm = np.float32(beta) * m
    c = round_clip(np.float32(alpha) * n.astype(np.float32) + bm)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    inv = np.asarray(inverse, np.float64)
    sx = (inv[0, 0] * xs + inv[0, 1] * ys) + inv[0, 2]
    sy = (inv[1, 0] * xs + inv[1, 1] * ys) + inv[1, 2]
    fixed_x = np.clip(np.floor(sx * 32.0 + 0.5), -2.0 ** 40, 2.0 ** 40).astype(np.int64)
    fixed_y = np.clip(np.floor(sy * 32.0 + 0.5), -2.0 ** 40, 2.0 ** 40).astype(np.int64)
    fx, fy = (fixed_x & 31)[..., None], (fixed_y & 31)[..., None]
    xa, xb = reflect101(fixed_x >> 5, w), reflect101((fixed_x >> 5) + 1, w)
    ya, yb = reflect101(fixed_y >> 5, h), reflect101((fixed_y >> 5) + 1, h)
    acc = (32 - fx) * (32 - fy) * c[ya, xa] + fx * (32 - fy) * c[ya, xb] + (32 - fx) * fy * c[yb, xa] + fx * fy * c[yb, xb]
    return ((acc + 512) >> 10).astype(np.uint8)


def restated_batch(resized_u8, table):
    return np.stack([restated_augment(resized_u8[i], table.noise_sigma[i], table.noise_seed[i], table.alpha[i], table.beta[i],
                                      table.inverse[i]) for i in range(resized_u8.shape[0])])


def restated_keypoints(kps_raw, table, raw, net_in, net_out, mode):
    """-> (netin float64, netout float32) [B,K,2]: host mirrors, k' = M k in float64 for non-identity rows."""
    netin, netout = [], []
    for i, k in enumerate(kps_raw):
        k_in = np.asarray(image_proc.convert_keypoints_to_netin_from_raw(k, raw, net_in, mode), np.float64)
        m = None if table is None else table.matrix[i]
        if m is not None and not np.array_equal(m, [[1, 0, 0], [0, 1, 0]]):
            k_in = np.stack([(m[0, 0] * k_in[:, 0] + m[0, 1] * k_in[:, 1]) + m[0, 2],
                             (m[1, 0] * k_in[:, 0] + m[1, 1] * k_in[:, 1]) + m[1, 2]], axis=1)
        netin.append(k_in)
        netout.append(image_proc.convert_keypoints_to_netout_from_netin(k_in, net_in, net_out).astype(np.float32))
    return np.stack(netin), np.stack(netout)


def host_belief_maps(netout32, net_out):
    """create_belief_map as the reference defines it (image_proc.py:866-910), on float32 keypoints, as float32."""
    ow, oh = net_out
    out = np.zeros(netout32.shape[:2] + (oh, ow), np.float32)
    dy, dx = np.mgrid[-4:5, -4:5]
    blob = np.exp(-((dx ** 2 + dy ** 2) / (2 * (2 ** 2)))).astype(np.float32)
    for b in range(netout32.shape[0]):
        for j, (x, y) in enumerate(netout32[b]):
            u, v = int(x), int(y)
            if u - 4 >= 0 and u + 5 < ow and v - 4 >= 0 and v + 5 < oh:
                out[b, j, v - 4:v + 5, u - 4:u + 5] = blob
    return out


def mixed_table(b, net_in, seed=5):
    """Rows of every kind: off, each stage alone, all three, a 90-degree rotation, a shift larger than the frame, clipping noise."""
    w, h = net_in
    ssr = image_proc.shift_scale_rotate_matrix
    rows = [dict(),
            dict(noise_sigma=5.0, noise_seed=123456789),
            dict(alpha=1.15, beta=-0.12),
            dict(matrix=ssr(net_in, 0.05, -0.03, 1.08, 11.0)),
            dict(noise_sigma=6.5, noise_seed=4294967295, alpha=0.83, beta=0.19, matrix=ssr(net_in, -0.06, 0.04, 0.92, -14.0)),
            dict(matrix=ssr(net_in, 0.0, 0.0, 1.0, 90.0)),
            dict(matrix=np.array([[1.0, 0.0, 2.5 * w + 0.3], [0.0, 1.0, -3.25 * h]])),
            dict(noise_sigma=400.0, noise_seed=seed)]
    rows = [rows[i % len(rows)] for i in range(b)]
    return image_proc.AugmentationTable(
        b, [r.get("noise_sigma", 0.0) for r in rows], [r.get("noise_seed", 0) for r in rows], [r.get("alpha", 1.0) for r in rows],
        [r.get("beta", 0.0) for r in rows], np.stack([r.get("matrix", np.array([[1.0, 0, 0], [0, 1.0, 0]])) for r in rows]))


# ---- host mirrors, fixture, sampler (no kernels) ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mtf.CASES))
def test_host_mirrors_match_reference_fixture(name):
    gold = np.load(mtf.OUT)
    b, raw, net_in, net_out, mode, _, _ = mtf.CASES[name]
    kps = mtf.keypoints(name)
    assert np.array_equal(kps, gold[name + ".raw"])
    for i in range(b):
        k_in = image_proc.convert_keypoints_to_netin_from_raw(kps[i], raw, net_in, mode)
        k_out = image_proc.convert_keypoints_to_netout_from_netin(k_in, net_in, net_out)
        assert isinstance(k_in, np.ndarray) and isinstance(k_out, np.ndarray) and k_out.dtype == np.float64
        assert np.array_equal(k_in, gold[name + ".netin"][i]) and np.array_equal(k_out, gold[name + ".netout"][i])
        assert np.array_equal(k_out.astype(np.float32), gold[name + ".netout32"][i])
    assert np.array_equal(host_belief_maps(gold[name + ".netout32"], net_out), gold[name + ".belief_maps"])


def test_fixture_holds_the_float32_boundary_and_border_points():
    gold = np.load(mtf.OUT)
    out64, out32, maps = gold["vga_crop.netout"][0], gold["vga_crop.netout32"][0], gold["vga_crop.belief_maps"][0]
    j = 7                                                   # raw (195.2, 278.4)
    assert out64[j, 0] == 23.999999999999996 and out64[j, 1] == 57.99999999999999 and tuple(out32[j]) == (24.0, 58.0)
    assert maps[j, 58, 24] == 1.0 and maps[j, 57, 23] < 1.0           # the blob sits where the float32 cast puts it
    assert not maps[0:4].any() and all(maps[i].max() == 1.0 for i in (4, 5, 6))    # windows touching each border: all zero
    assert (gold["vga_crop.netin"][0][8, 0] < 0) and not maps[8].any()             # inside the raw frame, outside the crop
    assert (gold["vga_crop.raw"][0][9] < 0).all() and not maps[9].any() and not maps[10].any()      # negative; outside the frame


@pytest.mark.skipif(not have_reference(), reason="the reference checkout is not on this machine")
def test_fixture_regenerates_byte_identical():
    with open(mtf.OUT, "rb") as f:
        assert mtf.fixture_bytes() == f.read()


def test_sampler_is_reproducible_and_within_limits():
    n, res = 12000, (400, 300)
    a = image_proc.sample_augmentation(n, res, np.random.RandomState(3))
    b = image_proc.sample_augmentation(n, res, np.random.RandomState(3))
    assert np.array_equal(a.packed(), b.packed())
    assert not np.array_equal(a.packed(), image_proc.sample_augmentation(n, res, np.random.RandomState(4)).packed())
    g = image_proc.sample_augmentation(64, res, np.random.default_rng(3))         # a Generator works too
    assert g.packed().shape == (64, 16) and np.isfinite(g.packed()).all()
    noisy = a.noise_sigma > 0
    bc = (a.alpha != 1) | (a.beta != 0)
    warped = ~(a.matrix == np.array([[1.0, 0, 0], [0, 1.0, 0]])).all(axis=(1, 2))
    for share in (noisy.mean(), bc.mean(), warped.mean()):
        assert abs(share - 0.5) <= 5 * np.sqrt(0.25 / n)
    var = a.noise_sigma[noisy].astype(np.float64) ** 2
    assert var.min() >= 10 * (1 - 1e-6) and var.max() <= 50 * (1 + 1e-6)
    assert np.abs(a.alpha - 1).max() <= np.float32(0.2) + 1e-7 and np.abs(a.beta).max() <= np.float32(0.2) + 1e-7
    m = a.matrix[warped]
    scale = np.sqrt(m[:, 0, 0] ** 2 + m[:, 0, 1] ** 2)
    angle = np.degrees(np.arctan2(m[:, 0, 1], m[:, 0, 0]))
    assert np.abs(scale - 1).max() <= 0.1 + 1e-12 and np.abs(angle).max() <= 15 + 1e-9
    centre = np.array([(res[0] - 1) / 2, (res[1] - 1) / 2, 1.0])
    shift = (m @ centre - centre[:2]) / np.array(res, float)                        # the centre moves by the shift alone
    assert np.abs(shift).max() <= 0.0625 + 1e-12
    fwd = np.concatenate([a.matrix, np.tile([[[0, 0, 1.0]]], (n, 1, 1))], axis=1)
    inv = np.concatenate([a.inverse, np.tile([[[0, 0, 1.0]]], (n, 1, 1))], axis=1)
    assert np.abs(fwd @ inv - np.eye(3)).max() <= 1e-12
    off = image_proc.sample_augmentation(8, res, np.random.RandomState(1), p=0.0)
    assert np.array_equal(off.packed(), image_proc.AugmentationTable(8, noise_seed=off.noise_seed).packed())


def test_restated_noise_statistics_without_kernels():
    """The definition itself: mean and standard deviation of the noise on a constant frame (three seeds)."""
    u = np.full((100, 100, 3), 128, np.uint8)
    for seed in (1, 77, 4000000000):
        d = restated_noise(u, 5.0, seed) - 128
        assert abs(d.mean()) <= 5 * 5.0 / np.sqrt(d.size) and abs(d.std() / 5.0 - 1) <= 0.03


# ---- the kernels under the SIMT emulator ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """A library of this module's own (see test_frame_preprocess.py: another pytest process may rebuild the shared one)."""
    import build_emu
    shared = build_emu.OUT
    build_emu.OUT = str(tmp_path_factory.mktemp("emu") / "libdream_emu.so")
    try:
        with emulated_hip() as lib:
            yield lib
    finally:
        build_emu.OUT = shared


def prepare(name, augmentation=None, frames=None, keypoints=None):
    _, _, net_in, net_out, mode, _, _ = mtf.CASES[name]
    frames = mtf.frames(name) if frames is None else frames
    keypoints = mtf.keypoints(name) if keypoints is None else keypoints
    return image_proc.training_batch_from_frames(frames, keypoints, net_in, net_out, mode, MEAN, STDEV, augmentation=augmentation,
                                                 return_u8=True)


@pytest.mark.parametrize("name", list(mtf.CASES))
def test_emulated_batch_without_augmentation(emu, name):
    gold = np.load(mtf.OUT)
    _, _, net_in, _, mode, _, _ = mtf.CASES[name]
    frames = mtf.frames(name)
    batch = prepare(name)
    pil = mfp.pil_preprocess(frames, net_in, mode)
    x, _ = image_proc.preprocess_frames(frames, net_in, mode, MEAN, STDEV)
    assert batch["image_rgb_input"].dtype == torch.float32
    assert torch.equal(batch["image_rgb_input"], x) and torch.equal(x, host_input(pil))
    assert np.array_equal(batch["image_rgb_input_u8"].numpy(), pil)
    assert batch["keypoint_projections_output"].dtype == torch.float32 and batch["keypoint_projections_input"].dtype == torch.float64
    assert np.array_equal(batch["keypoint_projections_input"].numpy(), gold[name + ".netin"])
    assert np.array_equal(batch["keypoint_projections_output"].numpy(), gold[name + ".netout32"])
    assert batch["belief_maps"].dtype == torch.float32 and np.array_equal(batch["belief_maps"].numpy(), gold[name + ".belief_maps"])
    assert "belief_maps" not in image_proc.training_batch_from_frames(
        frames, mtf.keypoints(name), net_in, (12, 12), mode, MEAN, STDEV, include_belief_maps=False)


@pytest.mark.parametrize("name", ["small_crop", "small_resize"])
def test_emulated_identity_rows_equal_no_augmentation(emu, name):
    b = mtf.CASES[name][0]
    plain, off = prepare(name), prepare(name, image_proc.AugmentationTable(b, noise_seed=np.arange(b) + 9))
    for key in plain:
        assert torch.equal(plain[key], off[key]), key


def augmentation_case(name, b):
    """A batch of b frames of the case's size: frame 0 constant grey 128, the others seeded noise; keypoints tiled."""
    _, (w, h), _, _, _, seed, _ = mtf.CASES[name]
    frames = np.random.RandomState(seed + 50).randint(0, 256, (b, h, w, 3)).astype(np.uint8)
    kps = np.concatenate([mtf.keypoints(name)] * b)[:b]
    return frames, kps


@pytest.mark.parametrize("name", ["small_crop", "small_resize"])
def test_emulated_augmentation_matches_restatement(emu, name):
    _, raw, net_in, net_out, mode, _, _ = mtf.CASES[name]
    b = 8
    frames, kps = augmentation_case(name, b)
    table = mixed_table(b, net_in)
    got = prepare(name, table, frames, kps)
    resized = mfp.pil_preprocess(frames, net_in, mode)
    want_u8 = restated_batch(resized, table)
    assert np.array_equal(got["image_rgb_input_u8"].numpy(), want_u8)
    assert torch.equal(got["image_rgb_input"], host_input(want_u8))
    assert np.array_equal(want_u8[0], resized[0]) and all((want_u8[i] != resized[i]).any() for i in range(1, b))
    sat = restated_noise(resized[7], 400.0, 5)
    assert (sat == 0).any() and (sat == 255).any()                      # the last row clips at both ends
    netin, netout = restated_keypoints(kps, table, raw, net_in, net_out, mode)
    assert np.array_equal(got["keypoint_projections_input"].numpy(), netin)
    assert np.array_equal(got["keypoint_projections_output"].numpy(), netout)
    assert np.array_equal(got["belief_maps"].numpy(), host_belief_maps(netout, net_out))
    # each frame alone with its own row; a second call with the same table
    again = prepare(name, table, frames, kps)
    for key in got:
        assert torch.equal(got[key], again[key]), key
    for i in range(b):
        one = prepare(name, table.row(i), frames[i:i + 1], kps[i:i + 1])
        for key in got:
            assert torch.equal(one[key][0], got[key][i]), (key, i)


def test_emulated_noise_statistics(emu):
    frames = np.full((1, 100, 100, 3), 128, np.uint8)
    table = image_proc.AugmentationTable(1, noise_sigma=[5.0], noise_seed=[20240229])
    x, u8 = image_proc.augment_frames_u8(torch.from_numpy(frames), table, MEAN, STDEV, return_u8=True)
    d = u8.numpy().astype(np.float64) - 128
    assert d.size >= 3e4 and abs(d.mean()) <= 5 * 5.0 / np.sqrt(d.size) and abs(d.std() / 5.0 - 1) <= 0.03
    assert np.array_equal(u8.numpy()[0], restated_augment(frames[0], 5.0, 20240229, 1.0, 0.0, [[1, 0, 0], [0, 1, 0]]))
