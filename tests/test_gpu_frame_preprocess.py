"""GPU suite (-m gpu): image_proc.preprocess_frames and DreamNetwork.keypoints_from_frames on an MI355X, bit for bit against
Pillow (live and the committed fixture) at real camera sizes, and against the host path of keypoints_from_image."""
import numpy as np
import pytest
import torch
from PIL import Image

import make_frame_preprocess as mfp
from dream_amd import _hip, image_proc
from test_frame_preprocess import MEAN, STDEV, host_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_library():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _hip.check_symbols()
    yield


def check_against_pil(frames, ref, mode):
    x, res, u8 = image_proc.preprocess_frames(torch.from_numpy(frames).cuda(), ref, mode, MEAN, STDEV, return_u8=True)
    assert x.is_cuda and u8.is_cuda
    pil = mfp.pil_preprocess(frames, ref, mode)
    assert res == (pil.shape[2], pil.shape[1])
    assert np.array_equal(u8.cpu().numpy(), pil), (frames.shape, mode)
    assert torch.equal(x.cpu(), host_input(pil)), (frames.shape, mode)
    return x


@pytest.mark.parametrize("mode", ["resize", "shrink", "shrink-and-crop"])
@pytest.mark.parametrize("w,h", [(640, 480), (1280, 720), (1920, 1080)])
def test_real_sizes_bit_exact(w, h, mode):
    frames = np.random.RandomState(w + h).randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    check_against_pil(frames, (400, 400), mode)


def test_batch128_640x480():
    rs = np.random.RandomState(128)
    frames = rs.randint(0, 256, (128, 480, 640, 3)).astype(np.uint8)
    x = check_against_pil(frames, (400, 400), "shrink-and-crop")
    assert tuple(x.shape) == (128, 3, 400, 400)


@pytest.mark.parametrize("name", list(mfp.CASES))
def test_fixture_cases(name):
    gold = np.load(mfp.OUT)
    _, _, _, ref, mode, _ = mfp.CASES[name]
    x, _, u8 = image_proc.preprocess_frames(torch.from_numpy(gold[name + ".frames"]).cuda(), ref, mode, MEAN, STDEV,
                                            return_u8=True)
    assert np.array_equal(u8.cpu().numpy(), gold[name + ".pil"]), name
    assert torch.equal(x.cpu(), host_input(gold[name + ".pil"])), name


def structured_frames():
    """Two raw 400 x 300 frames on which the vgg_q network of structured_network() detects keypoints: the structured
    fixture's 200 x 200 frames (uint8, recovered exactly from their Normalize(0.5, 0.5) form) upscaled to 300 x 300 by PIL
    and centred on a grey background, so shrink-and-crop crops x 50..350 and resizes 300 -> 200."""
    import cases
    x, _ = cases.structured_input("vgg_q")
    u8 = np.rint((x.transpose(0, 2, 3, 1) * 0.5 + 0.5) * 255).astype(np.uint8)
    raw = np.full((2, 300, 400, 3), 128, np.uint8)
    for b in range(2):
        raw[b, :, 50:350] = np.asarray(Image.fromarray(u8[b]).resize((300, 300), Image.BILINEAR))
    return raw


def structured_network(dev):
    """vgg_q on the recipe weights with the structured fixture's last layer, trained input 200 x 200 (check_structured)."""
    import cases
    import parity_checks as pc
    from oracle import models as om
    g = cases.load_structured(mfp.HERE, "vgg_q")
    w = om.recipe_weights(om.build_model("vgg_q", 7).state_dict())
    w["heads_0.4.weight"] = torch.from_numpy(g["final_weight"])
    w["heads_0.4.bias"] = torch.from_numpy(g["final_bias"])
    net = pc.build_network("vgg_q", dev, weights=w, in_res=(200, 200))
    net.enable_evaluation()
    return net


def check_keypoints_from_frames(net, raw):
    """keypoints_from_frames == the host path on the same batch: per-frame PIL preprocessing + normalise stacked into one
    batch, inference(), the host conversions of keypoints_from_image."""
    b = raw.shape[0]
    got = net.keypoints_from_frames(raw, debug=True)
    pre = [image_proc.preprocess_image(Image.fromarray(f), net.trained_net_input_resolution(), net.image_preprocessing())
           for f in raw]
    pil = np.stack([np.asarray(p) for p in pre])
    assert np.array_equal(got["image_rgb_net_input"].cpu().numpy(), pil)
    norm = net.image_normalization
    host_x = torch.stack([torch.from_numpy(np.ascontiguousarray(
        ((np.asarray(p, np.float32) / np.float32(255.0) - np.asarray(norm["mean"], np.float32))
         / np.asarray(norm["stdev"], np.float32)).transpose(2, 0, 1))) for p in pre])
    dev_x, netin_res = image_proc.preprocess_frames(raw, net.trained_net_input_resolution(), net.image_preprocessing(),
                                                    norm["mean"], norm["stdev"])
    assert torch.equal(dev_x.cpu(), host_x) and netin_res == pre[0].size
    with torch.no_grad():
        maps, kps = net.inference(host_x)
    assert torch.equal(got["belief_maps"].cpu(), maps.cpu())
    netout_res = (maps.shape[3], maps.shape[2])
    raw_res = (raw.shape[2], raw.shape[1])
    for i in range(b):
        k_out = np.array(kps[i].numpy(), dtype=float)
        k_in = image_proc.convert_keypoints_to_netin_from_netout(k_out, netout_res, netin_res)
        k_raw = image_proc.convert_keypoints_to_raw_from_netin(k_in, netin_res, raw_res, net.image_preprocessing())
        assert np.array_equal(got["detected_keypoints_net_output"][i], k_out)
        assert np.array_equal(got["detected_keypoints_net_input"][i], k_in)
        assert np.array_equal(got["detected_keypoints"][i], k_raw)
    assert got["detected_keypoints"].dtype == np.float64 and got["detected_keypoints"].shape == (b, 7, 2)
    return got


@pytest.fixture(scope="module")
def net():
    return structured_network("cuda")


def test_keypoints_from_frames_vgg_q(net):
    raw = structured_frames()
    got = check_keypoints_from_frames(net, raw)
    det = got["detected_keypoints"][..., 0] > -999
    assert det.any() and not det.all()               # detections and sentinels both covered
    # device input, hipGraph replay: same result
    net.hip_graph = True
    try:
        again = net.keypoints_from_frames(torch.from_numpy(raw).cuda())
        again2 = net.keypoints_from_frames(torch.from_numpy(raw).cuda())
    finally:
        net.hip_graph = False
    assert np.array_equal(again["detected_keypoints"], got["detected_keypoints"])
    assert np.array_equal(again2["detected_keypoints"], got["detected_keypoints"])


def test_keypoints_from_frames_single_frame_equals_keypoints_from_image(net):
    raw = structured_frames()
    for b in range(raw.shape[0]):
        got = net.keypoints_from_frames(raw[b:b + 1])
        one = net.keypoints_from_image(Image.fromarray(raw[b]))
        assert np.array_equal(got["detected_keypoints"][0], one["detected_keypoints"]), b
        assert (one["detected_keypoints"][:, 0] > -999).any()
