"""Generator of training_frames.npz: what the reference's own keypoint chain of ManipulatorNDDSDataset.__getitem__
(dream/datasets.py:135-207: convert_keypoints_to_netin_from_raw -> convert_keypoints_to_netout_from_netin -> .float() ->
create_belief_map -> .float()) produces for seeded raw keypoints, over all four preprocessing types.  Data only: the
reference is imported through ref_import.py and called; the tests of image_proc.training_batch_from_frames compare against
the recorded arrays.

    python tests/golden/make_training_frames.py          # rewrites training_frames.npz (needs the reference checkout)
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "training_frames.npz")

# name -> (batch, raw (w, h), net input (w, h), net output (w, h), preprocessing, seed, random keypoints per frame)
CASES = {
    "vga_none": (1, (640, 480), (400, 400), (100, 100), "none", 11, 4),
    "vga_resize": (1, (640, 480), (400, 400), (100, 100), "resize", 12, 4),
    "vga_shrink": (1, (640, 480), (400, 400), (100, 100), "shrink", 13, 4),
    "vga_crop": (1, (640, 480), (400, 400), (100, 100), "shrink-and-crop", 14, 4),
    "small_crop": (3, (46, 30), (16, 16), (12, 12), "shrink-and-crop", 15, 5),        # frames small enough for the SIMT emulator
    "small_resize": (2, (33, 25), (20, 14), (14, 10), "resize", 16, 5),
}

# raw keypoints (in 640 x 480 pixels, scaled to the case's raw frame) every case carries besides the designed net-output
# positions of keypoints()
FIXED_RAW_VGA = [
    (195.2, 278.4),        # shrink-and-crop: 23.999999999999996 / 57.99999999999999 in float64, 24.0 / 58.0 as float32
    (40.0, 200.0),         # inside the raw frame, outside the crop window (x < 80)
    (-12.5, -3.25),        # negative coordinates
    (700.0, 500.0),        # outside the frame
    (639.999, 479.999),
]


def frames(name):
    b, (w, h), _, _, _, seed, _ = CASES[name]
    return np.random.RandomState(seed).randint(0, 256, (b, h, w, 3)).astype(np.uint8)


def keypoints(name):
    """Raw keypoints [B,K,2] float64 of a case: net-output positions whose blob window (2 sigma = 4 pixels, plus one) touches the
    left / right / top / bottom border (all-zero maps), the first positions where it fits and the centre, mapped back to the raw
    frame in float64; the fixed raw points above; seeded random ones from inside and around the frame."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from dream_amd import image_proc
    b, raw, net_in, net_out, mode, seed, n_random = CASES[name]
    rs = np.random.RandomState(seed + 100)
    ow, oh = net_out
    netout = [(3.5, oh / 2), (ow - 4.5, oh / 2), (ow / 2, 3.5), (ow / 2, oh - 4.5), (4.5, 4.5), (ow - 5.5, oh - 5.5),
              (ow / 2 + 0.25, oh / 2 + 0.75)]
    target = image_proc.resolution_after_preprocessing(raw, net_in, mode)
    netin = np.array(netout) / np.array(net_out, float) * np.array(net_in, float)
    designed = image_proc.convert_keypoints_to_raw_from_netin(netin, target if mode == "shrink" else net_in, raw, mode)
    fixed = np.array(FIXED_RAW_VGA) * (np.array(raw, float) / np.array([640.0, 480.0]))
    out = []
    for _ in range(b):
        rnd = np.stack([rs.uniform(-0.1 * raw[0], 1.1 * raw[0], n_random), rs.uniform(-0.1 * raw[1], 1.1 * raw[1], n_random)], 1)
        out.append(np.concatenate([designed, fixed, rnd]))
    return np.stack(out).astype(np.float64)


def reference_chain(name):
    """The reference's functions chained as datasets.py:135-207 chains them, per frame."""
    import torch
    import ref_import
    dream = ref_import.import_reference()
    b, raw, net_in, net_out, mode, _, _ = CASES[name]
    kps = keypoints(name)
    netin, netout, netout32, maps = [], [], [], []
    for i in range(b):
        k_in = dream.image_proc.convert_keypoints_to_netin_from_raw([list(p) for p in kps[i]], raw, net_in, mode)
        k_out = dream.image_proc.convert_keypoints_to_netout_from_netin(k_in, net_in, net_out)
        k_out_t = torch.from_numpy(np.array(k_out)).float()
        m = torch.tensor(dream.image_proc.create_belief_map(net_out, k_out_t)).float()
        netin.append(np.array(k_in, np.float64))
        netout.append(np.array(k_out, np.float64))
        netout32.append(k_out_t.numpy())
        maps.append(m.numpy())
    return {"raw": kps, "netin": np.stack(netin), "netout": np.stack(netout), "netout32": np.stack(netout32),
            "belief_maps": np.stack(maps)}


def fixture_bytes():
    """The .npz file as bytes: fixed member order and time stamps, so the same reference always writes the same file."""
    arrays = {}
    for name in CASES:
        for key, value in reference_chain(name).items():
            arrays[name + "." + key] = value
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
    sys.path.insert(0, HERE)
    data = fixture_bytes()
    with open(OUT, "wb") as f:
        f.write(data)
    print("%s: %d bytes" % (OUT, len(data)))
