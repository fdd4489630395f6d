"""Generator of frame_preprocess.npz: seeded uint8 RGB frames and what Pillow's crop + resize(BILINEAR) makes of them
(dream_amd.image_proc.preprocess_image, the per-frame path of keypoints_from_image) for each preprocessing mode.  The
fixture pins the expected bytes for the tests of image_proc.preprocess_frames even where another Pillow is installed.

    python tests/golden/make_frame_preprocess.py          # rewrites frame_preprocess.npz (byte-identical for one Pillow)
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "frame_preprocess.npz")

# name -> (batch, raw height, raw width, net input resolution (w, h), preprocessing, seed).  Extents stay in the tens of
# pixels: the CPU suite runs the kernel under the SIMT emulator.
CASES = {
    "landscape_crop": (1, 30, 46, (16, 16), "shrink-and-crop", 1),         # crop in x, downscale 1.875
    "portrait_crop": (1, 47, 24, (12, 12), "shrink-and-crop", 2),          # crop in y
    "odd_corner": (1, 20, 35, (10, 10), "shrink-and-crop", 3),             # crop corner x0 = 7
    "upscale": (1, 9, 13, (20, 20), "resize", 4),                          # raw smaller than the net input
    "one_axis": (1, 16, 40, (16, 16), "resize", 5),                        # only x changes
    "identity": (1, 16, 40, (16, 16), "shrink", 6),                        # 40 x 16 -> 40 x 16
    "batch3": (3, 25, 33, (14, 14), "shrink", 7),                          # three different frames
    "ragged_tiles": (1, 24, 100, (70, 37), "resize", 8),                   # 2 column tiles (64 + 6), 37 rows
    "downscale_4x": (1, 40, 60, (10, 10), "shrink-and-crop", 9),           # 40 -> 10: ksize 9
}


def frames(name):
    b, h, w, _, _, seed = CASES[name]
    return np.random.RandomState(seed).randint(0, 256, (b, h, w, 3)).astype(np.uint8)


def pil_preprocess(frames_bhwc, ref, mode):
    """Pillow's bytes for each frame (the host path: preprocess_image on a PIL RGB image)."""
    from PIL import Image
    from dream_amd import image_proc
    return np.stack([np.asarray(image_proc.preprocess_image(Image.fromarray(f), ref, mode).convert("RGB")) for f in frames_bhwc])


def fixture_bytes():
    """The .npz file as bytes: fixed member order and time stamps, so one Pillow always writes the same file."""
    import PIL
    arrays = {"pillow_version": np.array(PIL.__version__)}
    for name, (_, _, _, ref, mode, _) in CASES.items():
        f = frames(name)
        arrays[name + ".frames"] = f
        arrays[name + ".pil"] = pil_preprocess(f, ref, mode)
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, member.getvalue())
    return buf.getvalue()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    data = fixture_bytes()
    with open(OUT, "wb") as f:
        f.write(data)
    print("%s: %d bytes" % (OUT, len(data)))
