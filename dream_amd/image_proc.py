"""Host-side mirror of the parts of /root/reference/dream/image_proc.py that sit on the hot path or
directly beside it: ``peaks_from_belief_maps`` (image_proc.py:914-1018, runs on the GPU here), the
resolution arithmetic DreamNetwork needs (image_proc.py:94-133, 291-351) and the keypoint frame
conversions used by ``keypoints_from_image`` (image_proc.py:135-260)."""
import numpy as np
import torch
from PIL import Image as PILImage

from . import _hip, ops

KNOWN_IMAGE_PREPROC_TYPES = ["none", "resize", "shrink", "shrink-and-crop"]

# scipy.ndimage._filters._gaussian_kernel1d(sigma=3, order=0, radius=12)[0:13] as float64 hex: the 13
# distinct taps hard-coded in csrc/peaks.hip (index 12 = centre).  tests/test_oracle_peaks.py checks
# that the installed scipy/numpy would compute exactly these.
GAUSS_SIGMA3_HALF_TAPS_HEX = (
    "0x1.763a210dfb306p-15", "0x1.4fbe39149e277p-13", "0x1.0d8a5ad43c165p-11", "0x1.8345966f69518p-10",
    "0x1.f1e9915139406p-9", "0x1.1e6bccad344bap-7", "0x1.26defcaeb0202p-6", "0x1.0fa58939b528fp-5",
    "0x1.bfde9c12bec92p-5", "0x1.4a614d1afd337p-4", "0x1.b42a57d56c0bep-4", "0x1.01a25f86eb137p-3",
    "0x1.105a329f98197p-3")


def peaks_from_belief_maps(belief_map_tensor, offset_due_to_upsampling):
    """[N,H,W] tensor -> list (len N) of lists of (x, y, score, id), exactly the reference's return
    value (float64 centroids, float32 scores, running ids), computed by the HIP peak kernels."""
    assert (
        len(belief_map_tensor.shape) == 3
    ), "Expected belief_map_tensor to have shape [N x height x width], but it is {}.".format(belief_map_tensor.shape)
    maps = _hip.device_tensor(belief_map_tensor.detach())
    xy, score, counts = ops.peaks_list(maps.float(), offset_due_to_upsampling)
    xy, score, counts = xy.cpu().numpy(), score.cpu().numpy(), counts.cpu().numpy()
    all_peaks, counter = [], 0
    for j in range(maps.shape[0]):
        n = int(counts[j])
        all_peaks.append([(xy[j, i, 0], xy[j, i, 1], score[j, i], counter + i) for i in range(n)])
        counter += n
    return all_peaks


# ---- resolution arithmetic (image_proc.py:94-133, 300-351) ---------------------------------------------
def shrink_resolution(image_input_resolution, image_ref_resolution):
    factor = float(image_ref_resolution[1]) / float(image_input_resolution[1])
    return (int(image_input_resolution[0] * factor), image_ref_resolution[1])


def shrink_and_crop_resolution(image_input_resolution, image_ref_resolution):
    """-> ((cropped width, cropped height), (crop x0, crop y0)) in input pixels: the largest centred
    window of the input with the reference aspect ratio (same int() truncations as
    image_proc.py:317-351, so (640,480) vs (400,400) gives ((480,480),(80,0)))."""
    in_w, in_h = image_input_resolution
    ref_w, ref_h = image_ref_resolution
    h_from_w = int(float(in_w) / float(ref_w) * ref_h)
    w_from_h = int(float(in_h) / float(ref_h) * ref_w)
    if in_w >= w_from_h:
        cropped = (w_from_h, in_h)
    else:
        assert in_h >= h_from_w
        cropped = (in_w, h_from_w)
    return cropped, ((in_w - cropped[0]) // 2, (in_h - cropped[1]) // 2)


def resolution_after_preprocessing(image_input_resolution, image_ref_resolution, image_preprocessing):
    assert (
        image_preprocessing in KNOWN_IMAGE_PREPROC_TYPES
    ), 'Image preprocessing type "{}" is not recognized.'.format(image_preprocessing)
    if image_preprocessing == "none":
        return image_input_resolution
    if image_preprocessing == "shrink":
        return shrink_resolution(image_input_resolution, image_ref_resolution)
    return image_ref_resolution              # resize, shrink-and-crop


def preprocess_image(input_image, image_ref_resolution, image_preprocessing):
    assert isinstance(input_image, PILImage.Image), 'Expected "input_image" to be a PIL Image, but it is "{}".'.format(
        type(input_image))
    assert image_preprocessing in KNOWN_IMAGE_PREPROC_TYPES, 'Image preprocessing type "{}" is not recognized.'.format(
        image_preprocessing)
    if image_preprocessing == "none":
        return input_image
    if image_preprocessing == "resize":
        return input_image.resize(image_ref_resolution, resample=PILImage.BILINEAR)
    if image_preprocessing == "shrink":
        return input_image.resize(shrink_resolution(input_image.size, image_ref_resolution), resample=PILImage.BILINEAR)
    (cw, ch), (x0, y0) = shrink_and_crop_resolution(input_image.size, image_ref_resolution)
    return input_image.crop((x0, y0, x0 + cw, y0 + ch)).resize(image_ref_resolution, resample=PILImage.BILINEAR)


# ---- keypoint frame conversions (image_proc.py:135-147, 215-260) ----------------------------------------
def convert_keypoints_to_netin_from_netout(keypoints_netout, net_output_resolution, net_input_resolution):
    k = np.asarray(keypoints_netout, dtype=float).reshape(-1, 2)
    return np.stack([k[:, 0] / net_output_resolution[0] * net_input_resolution[0],
                     k[:, 1] / net_output_resolution[1] * net_input_resolution[1]], axis=1)


def convert_keypoints_to_raw_from_netin(keypoints_netin, net_input_resolution, image_raw_resolution,
                                        image_preprocessing):
    assert image_preprocessing in KNOWN_IMAGE_PREPROC_TYPES, 'Image preprocessing type "{}" is not recognized.'.format(
        image_preprocessing)
    k = np.asarray(keypoints_netin, dtype=float).reshape(-1, 2)
    if image_preprocessing == "none":
        return k
    if image_preprocessing in ("resize", "shrink"):
        return np.stack([k[:, 0] / net_input_resolution[0] * image_raw_resolution[0],
                         k[:, 1] / net_input_resolution[1] * image_raw_resolution[1]], axis=1)
    (cw, ch), (x0, y0) = shrink_and_crop_resolution(image_raw_resolution, net_input_resolution)
    return np.stack([k[:, 0] / net_input_resolution[0] * cw + x0,
                     k[:, 1] / net_input_resolution[1] * ch + y0], axis=1)


def convert_keypoints_batch(keypoints_netout, net_output_resolution, net_input_resolution, image_raw_resolution,
                            image_preprocessing):
    """The two conversions above for a whole batch on the device: keypoints [..., 2] fp32 in the
    net-output frame (as DreamNetwork.inference computes them) -> (netin, raw) float64 tensors of the same shape, bit
    for bit what the per-keypoint Python loops of the reference produce (dream/analysis.py:219-232)."""
    assert image_preprocessing in KNOWN_IMAGE_PREPROC_TYPES, 'Image preprocessing type "{}" is not recognized.'.format(
        image_preprocessing)
    k = _hip.device_tensor(torch.as_tensor(keypoints_netout, dtype=torch.float32)).contiguous()
    n = k.numel() // 2
    netin = torch.empty(tuple(k.shape), dtype=torch.float64, device=k.device)
    raw = torch.empty_like(netin)
    (ow, oh), (iw, ih) = net_output_resolution, net_input_resolution
    if image_preprocessing == "none":
        mode, span, origin = 0, (1.0, 1.0), (0.0, 0.0)
    elif image_preprocessing in ("resize", "shrink"):
        mode, span, origin = 1, image_raw_resolution, (0.0, 0.0)
    else:
        span, origin = shrink_and_crop_resolution(image_raw_resolution, net_input_resolution)
        mode = 1
    _hip.call("dream_convert_keypoints_f64", ops.ptr(k), ops.ptr(netin), ops.ptr(raw), n, float(ow), float(oh), float(iw),
              float(ih), float(span[0]), float(span[1]), float(origin[0]), float(origin[1]), mode, ops.stream())
    return netin, raw


# ---- the steps right before the hot path, on the device ---------------------------------------
def normalize_images_u8(images_u8_bhwc, mean, stdev):
    """uint8 RGB frames [B,H,W,3] (device) -> normalised fp32 [B,3,H,W]: ToTensor + Normalize(mean, stdev) as the
    dataset does (dream/datasets.py:87-94), bit-identical to the torchvision transforms, without the 4x larger fp32
    upload."""
    import ctypes
    x = _hip.device_tensor(images_u8_bhwc)
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3, "expected uint8 [B,H,W,3]"
    x = x.contiguous()
    b, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=x.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in stdev])
    _hip.call("dream_normalize_u8_hwc_to_chw_f32", ops.ptr(x), ops.ptr(out), b, h, w, m, s, ops.stream())
    return out


def create_belief_map(image_resolution, pointsBelief, sigma=2):
    """Drop-in for dream/image_proc.py:866-910 (training targets, called per frame by dream/datasets.py:165-171):
    -> numpy float64 [n_points, H, W].  Rendered on the device by the batched kernel; every value is the fp32 rounding
    of the reference's float64 value, which is exactly what its only caller keeps (``torch.tensor(maps).float()``)."""
    assert len(image_resolution) == 2, \
        'Expected "image_resolution" to have length 2, but it has length {}.'.format(len(image_resolution))
    pts = np.asarray([[float(p[0]), float(p[1])] for p in pointsBelief], dtype=np.float64).reshape(-1, 2)
    if pts.shape[0] == 0:
        return np.zeros((0, int(image_resolution[1]), int(image_resolution[0])))
    maps = create_belief_map_batch(image_resolution, torch.from_numpy(pts)[None], sigma)
    return maps[0].cpu().numpy().astype(np.float64)


def create_belief_map_batch(image_resolution, keypoints_bk2, sigma=2):
    """Batched, on-device create_belief_map (dream/image_proc.py:866-910): keypoints [B,K,2] (x, y) in the belief-map
    frame -> fp32 [B,K,H,W], bit-identical to torch.tensor(create_belief_map(res, kps)).float() per frame."""
    assert len(image_resolution) == 2, \
        'Expected "image_resolution" to have length 2, but it has length {}.'.format(len(image_resolution))
    width, height = int(image_resolution[0]), int(image_resolution[1])
    # float64 all the way: the reference truncates the float64 coordinate with int() (image_proc.py:889-890)
    kps = _hip.device_tensor(torch.as_tensor(keypoints_bk2).to(torch.float64)).contiguous()
    b, k = int(kps.shape[0]), int(kps.shape[1])
    w = int(sigma * 2)
    dy, dx = np.mgrid[-w:w + 1, -w:w + 1]
    blob64 = np.exp(-((dx ** 2 + dy ** 2) / (2 * (sigma ** 2))))           # float64, as the reference computes it
    blob = torch.from_numpy(blob64.astype(np.float32)).to(kps.device)        # the .float() cast of the reference
    out = torch.empty((b, k, height, width), dtype=torch.float32, device=kps.device)
    _hip.call("dream_create_belief_maps_f64kps_f32", ops.ptr(kps), ops.ptr(blob), ops.ptr(out), b * k, height, width, w, ops.stream())
    return out


# ---- raw frames -> network input on the device (image_proc.py:26-51, 291-351; network.py:449-459) -------------------
PREPROCESS_TILE_W = 64          # output columns per workgroup of dream_preprocess_frames_u8_f32
PREPROCESS_LDS_BUDGET = 32768   # LDS bytes the planner aims at per workgroup (the entry point accepts up to 64 KiB)


def resample_coefficients(n_in, n_out):
    """Pillow's BILINEAR coefficients for one axis of an 8-bit image (Resample.c precompute_coeffs +
    normalize_coeffs_8bpc), in float64 as Pillow computes them: n_in input pixels (the cropped extent) -> n_out.
    -> (bounds int32 [n_out, 2] = (first input pixel, tap count), coeffs int32 [n_out, ksize] in units of 2^-22)."""
    scale = float(n_in) / float(n_out)
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), np.int32)
    coeffs = np.zeros((n_out, ksize), np.int32)
    for o in range(n_out):
        center = (o + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - lo
        w = []
        for i in range(n):
            t = abs((i + lo - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        for i, v in enumerate(w):
            v = v / ww if ww != 0.0 else v
            coeffs[o, i] = int(v * (1 << 22) + 0.5) if v >= 0 else int(v * (1 << 22) - 0.5)
        bounds[o] = (lo, n)
    return bounds, coeffs


def preprocess_geometry(image_raw_resolution, image_ref_resolution, image_preprocessing):
    """-> ((crop x0, y0, width, height), (out width, height)) of preprocess_image for a raw frame of this size."""
    assert image_preprocessing in KNOWN_IMAGE_PREPROC_TYPES, 'Image preprocessing type "{}" is not recognized.'.format(
        image_preprocessing)
    w, h = int(image_raw_resolution[0]), int(image_raw_resolution[1])
    if image_preprocessing == "shrink-and-crop":
        (cw, ch), (x0, y0) = shrink_and_crop_resolution((w, h), image_ref_resolution)
        crop = (x0, y0, cw, ch)
    else:
        crop = (0, 0, w, h)
    out = tuple(int(v) for v in resolution_after_preprocessing((w, h), image_ref_resolution, image_preprocessing))
    return crop, out


def _window(bounds, first, last):
    return int(bounds[last, 0] + bounds[last, 1] - bounds[first, 0])


def preprocess_plan(image_raw_resolution, image_ref_resolution, image_preprocessing):
    """Host side of dream_preprocess_frames_u8_f32 for one raw frame size: crop, output size, both axes' coefficient tables and
    the tiling (rows per workgroup, largest input window of a tile) -- numpy only, no device."""
    crop, (ow, oh) = preprocess_geometry(image_raw_resolution, image_ref_resolution, image_preprocessing)
    hb, hk = resample_coefficients(crop[2], ow)
    vb, vk = resample_coefficients(crop[3], oh)
    span_cols = max(_window(hb, x, min(x + PREPROCESS_TILE_W, ow) - 1) for x in range(0, ow, PREPROCESS_TILE_W))
    rs = (span_cols * 3 + 30) // 16 * 16                   # the kernel's LDS row: 16-byte chunks from an aligned address
    for tile_rows in (32, 16, 8, 4, 2, 1):
        span_rows = max(_window(vb, y, min(y + tile_rows, oh) - 1) for y in range(0, oh, tile_rows))
        lds = span_rows * (rs + 3 * PREPROCESS_TILE_W) + 4 * (PREPROCESS_TILE_W * (hk.shape[1] + 2) + tile_rows * (vk.shape[1] + 2))
        if lds <= PREPROCESS_LDS_BUDGET:
            break
    return {"crop": crop, "out": (ow, oh), "hbounds": hb, "hcoeffs": hk, "vbounds": vb, "vcoeffs": vk,
            "tile_rows": tile_rows, "span_rows": span_rows, "span_cols": span_cols}


_plans = {}


def _device_plan(device, image_raw_resolution, image_ref_resolution, image_preprocessing):
    key = (str(device), tuple(image_raw_resolution), tuple(image_ref_resolution), image_preprocessing)
    plan = _plans.get(key)
    if plan is None:
        plan = dict(preprocess_plan(image_raw_resolution, image_ref_resolution, image_preprocessing))
        for name in ("hbounds", "hcoeffs", "vbounds", "vcoeffs"):
            plan[name] = torch.from_numpy(np.ascontiguousarray(plan[name])).to(device)
        _plans[key] = plan
    return plan


def preprocess_frames(frames_u8_bhwc, image_ref_resolution, image_preprocessing, mean, stdev, return_u8=False):
    """Batched, on-device preprocess_image + ToTensor + Normalize(mean, stdev) of raw RGB frames of one size (the per-frame
    path is network.py:436-459): uint8 [B,H,W,3] (device or host tensor, or numpy array; host data is uploaded as uint8) ->
    (normalised fp32 [B,3,h,w] on the device, (w, h)[, resized uint8 [B,h,w,3]]).  The uint8 frames are bit for bit PIL's
    crop + resize(BILINEAR) and the fp32 tensor bit for bit what the host path computes from them."""
    out, res, u8 = _preprocess_frames(frames_u8_bhwc, image_ref_resolution, image_preprocessing, mean, stdev, True, return_u8)
    return (out, res, u8) if return_u8 else (out, res)


def _preprocess_frames(frames_u8_bhwc, image_ref_resolution, image_preprocessing, mean, stdev, want_f32, want_u8):
    """-> (fp32 network input or None, (w, h), resized uint8 frames or None); without the fp32 tensor the kernel skips its store."""
    import ctypes
    assert image_preprocessing in KNOWN_IMAGE_PREPROC_TYPES, 'Image preprocessing type "{}" is not recognized.'.format(
        image_preprocessing)
    x = frames_u8_bhwc
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3, "expected uint8 RGB frames [B,H,W,3]"
    x = _hip.device_tensor(x).contiguous()
    b, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    if image_preprocessing == "none":
        return (normalize_images_u8(x, mean, stdev) if want_f32 else None), (w, h), (x if want_u8 else None)
    if x.data_ptr() % 16:                       # the kernel reads the frames in aligned 16-byte chunks
        x = x.clone()
    plan = _device_plan(x.device, (w, h), image_ref_resolution, image_preprocessing)
    (ow, oh), (cx, cy, cw, ch) = plan["out"], plan["crop"]
    out = torch.empty((b, 3, oh, ow), dtype=torch.float32, device=x.device) if want_f32 else None
    u8 = torch.empty((b, oh, ow, 3), dtype=torch.uint8, device=x.device) if want_u8 else None
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in stdev])
    _hip.call("dream_preprocess_frames_u8_f32", ops.ptr(x), ops.ptr(out), ops.ptr(u8), b, h, w, cx, cy, cw, ch, oh, ow,
              ops.ptr(plan["hbounds"]), ops.ptr(plan["hcoeffs"]), int(plan["hcoeffs"].shape[1]), ops.ptr(plan["vbounds"]),
              ops.ptr(plan["vcoeffs"]), int(plan["vcoeffs"].shape[1]), plan["tile_rows"], plan["span_rows"], plan["span_cols"],
              m, s, ops.stream())
    return out, (ow, oh), u8


# ---- training batches from raw frames on the device (datasets.py:127-208) -------------------------------------------
def convert_keypoints_to_netout_from_netin(keypoints_netin, net_input_resolution, net_output_resolution):
    k = np.asarray(keypoints_netin, dtype=float).reshape(-1, 2)
    return np.stack([k[:, 0] / net_input_resolution[0] * net_output_resolution[0],
                     k[:, 1] / net_input_resolution[1] * net_output_resolution[1]], axis=1)


def _netin_from_raw_geometry(image_raw_resolution, net_input_resolution, image_preprocessing):
    """-> (origin, span, target) of netin = (raw - origin) / span * target (image_proc.py:176-209), None for "none"."""
    if image_preprocessing == "none":
        return None
    if image_preprocessing == "resize":
        return (0, 0), image_raw_resolution, net_input_resolution
    if image_preprocessing == "shrink":
        return (0, 0), image_raw_resolution, shrink_resolution(image_raw_resolution, net_input_resolution)
    span, origin = shrink_and_crop_resolution(image_raw_resolution, net_input_resolution)
    return origin, span, net_input_resolution


def convert_keypoints_to_netin_from_raw(keypoints_raw, image_raw_resolution, net_input_resolution, image_preprocessing):
    assert image_preprocessing in KNOWN_IMAGE_PREPROC_TYPES, 'Image preprocessing type "{}" is not recognized.'.format(
        image_preprocessing)
    geometry = _netin_from_raw_geometry(image_raw_resolution, net_input_resolution, image_preprocessing)
    if geometry is None:
        return np.array(keypoints_raw)
    origin, span, target = geometry
    k = np.asarray(keypoints_raw, dtype=float).reshape(-1, 2)
    if image_preprocessing == "shrink-and-crop":
        return np.stack([(k[:, 0] - origin[0]) / span[0] * target[0], (k[:, 1] - origin[1]) / span[1] * target[1]], axis=1)
    return np.stack([k[:, 0] / span[0] * target[0], k[:, 1] / span[1] * target[1]], axis=1)


AUGMENTATION_ROW = 16           # float64 values per frame of the packed parameter table (include/dream_hip.h)
NOISE_QUANTILES = 4096          # entries of the standard-normal quantile table the noise kernel indexes
_IDENTITY_2X3 = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


class AugmentationTable:
    """Per-frame augmentation parameters of a batch (the parameter table of DESIGN.md 4.4c), host arrays of length B:
    ``noise_sigma`` fp32 (0 = off) and ``noise_seed`` uint32; ``alpha`` / ``beta`` fp32 (contrast factor and brightness term in units
    of the frame's mean grey level; 1, 0 = off); ``matrix`` float64 [B,2,3], the forward affine map in net-input pixel
    coordinates (identity = off).  Omitted fields are off."""

    def __init__(self, batch_size, noise_sigma=None, noise_seed=None, alpha=None, beta=None, matrix=None):
        b = int(batch_size)

        def field(value, default, dtype, shape):
            a = np.full(shape, default, dtype) if value is None else np.ascontiguousarray(np.asarray(value).astype(dtype))
            assert a.shape == shape, "augmentation field of shape %s, expected %s" % (a.shape, shape)
            return a
        self.batch_size = b
        self.noise_sigma = field(noise_sigma, 0.0, np.float32, (b,))
        self.noise_seed = field(noise_seed, 0, np.uint32, (b,))
        self.alpha = field(alpha, 1.0, np.float32, (b,))
        self.beta = field(beta, 0.0, np.float32, (b,))
        self.matrix = np.tile(_IDENTITY_2X3, (b, 1, 1)) if matrix is None else field(matrix, 0.0, np.float64, (b, 2, 3))
        for a in (self.noise_sigma, self.alpha, self.beta, self.matrix):
            assert np.isfinite(a).all(), "augmentation parameters must be finite"
        assert (self.noise_sigma >= 0).all(), "noise_sigma must not be negative"

    @property
    def inverse(self):
        """float64 [B,2,3]: the inverse affine maps (output pixel -> source position), identity rows kept exact."""
        m = self.matrix
        det = m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0]
        assert (det != 0).all(), "augmentation matrix is singular"
        inv = np.empty_like(m)
        inv[:, 0, 0], inv[:, 0, 1] = m[:, 1, 1] / det, -m[:, 0, 1] / det
        inv[:, 1, 0], inv[:, 1, 1] = -m[:, 1, 0] / det, m[:, 0, 0] / det
        inv[:, 0, 2] = -(inv[:, 0, 0] * m[:, 0, 2] + inv[:, 0, 1] * m[:, 1, 2])
        inv[:, 1, 2] = -(inv[:, 1, 0] * m[:, 0, 2] + inv[:, 1, 1] * m[:, 1, 2])
        inv[(m == _IDENTITY_2X3).all(axis=(1, 2))] = _IDENTITY_2X3
        return inv

    def packed(self):
        """float64 [B,16] as the kernels read it: forward matrix, inverse, sigma, alpha, beta, seed."""
        t = np.empty((self.batch_size, AUGMENTATION_ROW), np.float64)
        t[:, 0:6] = self.matrix.reshape(-1, 6)
        t[:, 6:12] = self.inverse.reshape(-1, 6)
        t[:, 12], t[:, 13], t[:, 14], t[:, 15] = self.noise_sigma, self.alpha, self.beta, self.noise_seed
        return t

    def row(self, i):
        """The table of frame ``i`` alone (batch size 1)."""
        return AugmentationTable(1, self.noise_sigma[i:i + 1], self.noise_seed[i:i + 1], self.alpha[i:i + 1], self.beta[i:i + 1],
                                 self.matrix[i:i + 1])


def shift_scale_rotate_matrix(net_input_resolution, shift_x, shift_y, scale, angle_degrees):
    """float64 [2,3] forward map in net-input pixel coordinates: rotate by the angle (counter-clockwise on the screen) and scale about
    the frame centre ((w-1)/2, (h-1)/2), then shift by (shift_x * w, shift_y * h)."""
    w, h = net_input_resolution
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    a = np.deg2rad(angle_degrees)
    ca, sa = scale * np.cos(a), scale * np.sin(a)
    return np.array([[ca, sa, cx - ca * cx - sa * cy + shift_x * w],
                     [-sa, ca, cy + sa * cx - ca * cy + shift_y * h]])


def sample_augmentation(batch_size, net_input_resolution, rng, p=0.5, noise_var_limit=(10.0, 50.0), contrast_limit=0.2,
                        brightness_limit=0.2, shift_limit=0.0625, scale_limit=0.1, rotate_limit=15.0):
    """Draw an AugmentationTable on the host from ``rng`` (numpy RandomState or Generator; only ``rng.uniform`` is used, in a
    fixed order, so a seed reproduces the table).  Noise, brightness / contrast and shift-scale-rotate are each applied to a
    frame with probability ``p``; the limits are the defaults of the reference's albumentations call."""
    b = int(batch_size)
    on = rng.uniform(0.0, 1.0, (3, b)) < p
    var = rng.uniform(noise_var_limit[0], noise_var_limit[1], b)
    seed = np.minimum(np.floor(rng.uniform(0.0, 4294967296.0, b)), 4294967295.0).astype(np.uint32)
    alpha = 1.0 + rng.uniform(-contrast_limit, contrast_limit, b)
    beta = rng.uniform(-brightness_limit, brightness_limit, b)
    shift_x = rng.uniform(-shift_limit, shift_limit, b)
    shift_y = rng.uniform(-shift_limit, shift_limit, b)
    scale = 1.0 + rng.uniform(-scale_limit, scale_limit, b)
    angle = rng.uniform(-rotate_limit, rotate_limit, b)
    matrix = np.stack([shift_scale_rotate_matrix(net_input_resolution, shift_x[i], shift_y[i], scale[i], angle[i]) if on[2, i]
                       else _IDENTITY_2X3 for i in range(b)])
    return AugmentationTable(b, np.where(on[0], np.sqrt(var), 0.0), seed, np.where(on[1], alpha, 1.0), np.where(on[1], beta, 0.0),
                             matrix)


_quantiles = {}


def noise_quantiles():
    """fp32 [4096]: the standard-normal quantiles at the bin mid-points (i + 0.5) / 4096, computed in float64."""
    from statistics import NormalDist
    q = _quantiles.get("host")
    if q is None:
        inv = NormalDist().inv_cdf
        q = _quantiles["host"] = np.array([inv((i + 0.5) / NOISE_QUANTILES) for i in range(NOISE_QUANTILES)]).astype(np.float32)
    return q


def _device_quantiles(device):
    q = _quantiles.get(str(device))
    if q is None:
        q = _quantiles[str(device)] = torch.from_numpy(noise_quantiles()).to(device)
    return q


def augment_frames_u8(frames_u8_bhwc, augmentation, mean, stdev, return_u8=False):
    """Image half of the augmentation on resized uint8 net-input frames [B,h,w,3] (device): noise, brightness / contrast,
    shift-scale-rotate as DESIGN.md 4.4c defines them, then ToTensor + Normalize -> fp32 [B,3,h,w][, augmented uint8 frames]."""
    import ctypes
    x = _hip.device_tensor(frames_u8_bhwc).contiguous()
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3, "expected uint8 RGB frames [B,H,W,3]"
    b, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    table = _device_table(augmentation, b, x.device)
    g = int(_hip.lib().dream_augment_partials_per_frame(h, w))
    noised = torch.empty_like(x)
    partials = torch.empty((b * g,), dtype=torch.int64, device=x.device)
    frame_mean = torch.empty((b,), dtype=torch.float32, device=x.device)
    beta_mean = torch.empty_like(frame_mean)
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=x.device)
    u8 = torch.empty_like(x) if return_u8 else None
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in stdev])
    _hip.call("dream_augment_frames_u8_f32", ops.ptr(x), ops.ptr(table), ops.ptr(_device_quantiles(x.device)), ops.ptr(noised),
              ops.ptr(partials), ops.ptr(frame_mean), ops.ptr(beta_mean), ops.ptr(out), ops.ptr(u8), b, h, w, m, s, ops.stream())
    return (out, u8) if return_u8 else out


def _device_table(augmentation, batch_size, device):
    """The packed [B,16] float64 table on ``device``: from an AugmentationTable (one upload) or an already packed tensor."""
    t = augmentation.packed() if isinstance(augmentation, AugmentationTable) else augmentation
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    assert t.dtype == torch.float64 and tuple(t.shape) == (batch_size, AUGMENTATION_ROW), \
        "expected an AugmentationTable or a packed float64 [B,%d] table for %d frames" % (AUGMENTATION_ROW, batch_size)
    return (t if t.device == device else t.to(device)).contiguous()


def training_batch_from_frames(frames_u8_bhwc, keypoints_raw_bk2, net_input_resolution, net_output_resolution,
                               image_preprocessing, mean, stdev, augmentation=None, include_belief_maps=True, return_u8=False):
    """The batched, on-device twin of ManipulatorNDDSDataset.__getitem__ (datasets.py:127-208) for B raw RGB frames of one size:
    uint8 [B,H,W,3] (as preprocess_frames) and raw keypoints [B,K,2] float64 (x, y) in raw-frame pixels -> a dict of device
    tensors with the dataset's keys: "image_rgb_input" fp32 [B,3,h,w], "keypoint_projections_output" fp32 [B,K,2],
    "belief_maps" fp32 [B,K,Ho,Wo] (unless include_belief_maps is False), "keypoint_projections_input" float64 [B,K,2]
    (return_u8 adds "image_rgb_input_u8", the uint8 frames behind image_rgb_input).  ``augmentation``: None, an
    AugmentationTable or its packed float64 [B,16] form (a device tensor saves the upload).  Nothing synchronises with the
    host."""
    assert image_preprocessing in KNOWN_IMAGE_PREPROC_TYPES, 'Image preprocessing type "{}" is not recognized.'.format(
        image_preprocessing)
    x = frames_u8_bhwc
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3, "expected uint8 RGB frames [B,H,W,3]"
    x = _hip.device_tensor(x)
    b, raw_res = int(x.shape[0]), (int(x.shape[2]), int(x.shape[1]))
    kps = keypoints_raw_bk2
    if isinstance(kps, np.ndarray):
        kps = torch.from_numpy(np.ascontiguousarray(kps, dtype=np.float64))
    kps = _hip.device_tensor(torch.as_tensor(kps).to(torch.float64))
    kps = (kps if kps.device == x.device else kps.to(x.device)).contiguous()
    assert kps.dim() == 3 and kps.shape[0] == b and kps.shape[1] > 0 and kps.shape[2] == 2, "expected keypoints [B,K,2]"
    k = int(kps.shape[1])
    if augmentation is None:
        table = None
        image, _, u8 = _preprocess_frames(x, net_input_resolution, image_preprocessing, mean, stdev, True, return_u8)
    else:
        table = _device_table(augmentation, b, x.device)
        _, _, resized = _preprocess_frames(x, net_input_resolution, image_preprocessing, mean, stdev, False, True)
        image = augment_frames_u8(resized, table, mean, stdev, return_u8)
        image, u8 = image if return_u8 else (image, None)
    geometry = _netin_from_raw_geometry(raw_res, net_input_resolution, image_preprocessing)
    origin, span, target = geometry if geometry is not None else ((0, 0), (1, 1), (1, 1))
    netin = torch.empty((b, k, 2), dtype=torch.float64, device=x.device)
    netout = torch.empty((b, k, 2), dtype=torch.float32, device=x.device)
    netout64 = torch.empty_like(netin)
    _hip.call("dream_training_keypoints_f64", ops.ptr(kps), ops.ptr(table), ops.ptr(netin), ops.ptr(netout), ops.ptr(netout64), b, k,
              0 if geometry is None else 1, float(origin[0]), float(origin[1]), float(span[0]), float(span[1]), float(target[0]),
              float(target[1]), float(net_input_resolution[0]), float(net_input_resolution[1]), float(net_output_resolution[0]),
              float(net_output_resolution[1]), ops.stream())
    batch = {"image_rgb_input": image, "keypoint_projections_output": netout, "keypoint_projections_input": netin}
    if include_belief_maps:
        batch["belief_maps"] = create_belief_map_batch(net_output_resolution, netout64)
    if return_u8:
        batch["image_rgb_input_u8"] = u8
    return batch
