"""GPU suite (-m gpu): image_proc.training_batch_from_frames and DreamNetwork.train_from_frames / loss_from_frames on an MI355X,
bit for bit against Pillow, the host mirrors, the reference fixture and the NumPy restatement of the augmentation
(tests/test_training_frames.py) at real camera sizes."""
import numpy as np
import pytest
import torch

import make_frame_preprocess as mfp
import make_training_frames as mtf
from dream_amd import _hip, image_proc
from test_frame_preprocess import MEAN, STDEV, host_input
from test_training_frames import host_belief_maps, mixed_table, restated_batch, restated_keypoints

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_library():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _hip.check_symbols()
    yield


def raw_batch(b, w, h, k=7, seed=0):
    rs = np.random.RandomState(seed + w + h)
    frames = rs.randint(0, 256, (b, h, w, 3)).astype(np.uint8)
    kps = np.stack([rs.uniform(-0.05 * w, 1.05 * w, (b, k)), rs.uniform(-0.05 * h, 1.05 * h, (b, k))], axis=2)
    return frames, kps


def check_plain(frames, kps, net_in, net_out, mode, device_input):
    f, k = (torch.from_numpy(frames).cuda(), torch.from_numpy(kps).cuda()) if device_input else (frames, kps)
    got = image_proc.training_batch_from_frames(f, k, net_in, net_out, mode, MEAN, STDEV, return_u8=True)
    assert all(v.is_cuda for v in got.values())
    raw = (frames.shape[2], frames.shape[1])
    pil = mfp.pil_preprocess(frames, net_in, mode)
    x, _ = image_proc.preprocess_frames(f, net_in, mode, MEAN, STDEV)
    assert torch.equal(got["image_rgb_input"], x) and torch.equal(x.cpu(), host_input(pil))
    netin, netout = restated_keypoints(kps, None, raw, net_in, net_out, mode)
    assert np.array_equal(got["keypoint_projections_input"].cpu().numpy(), netin)
    assert np.array_equal(got["keypoint_projections_output"].cpu().numpy(), netout)
    assert np.array_equal(got["belief_maps"].cpu().numpy(), host_belief_maps(netout, net_out))
    return got


@pytest.mark.parametrize("mode", ["resize", "shrink-and-crop"])
@pytest.mark.parametrize("w,h", [(640, 480), (1280, 720), (1920, 1080)])
def test_real_sizes_without_augmentation(w, h, mode):
    frames, kps = raw_batch(2, w, h)
    check_plain(frames, kps, (400, 400), (100, 100), mode, device_input=(w == 640))
    check_plain(frames, kps, (208, 208), (52, 52), mode, device_input=True)              # resnet_h's resolutions


def test_batch128_without_augmentation():
    frames, kps = raw_batch(128, 640, 480)
    got = check_plain(frames, kps, (400, 400), (100, 100), "shrink-and-crop", device_input=False)
    assert tuple(got["image_rgb_input"].shape) == (128, 3, 400, 400) and tuple(got["belief_maps"].shape) == (128, 7, 100, 100)


@pytest.mark.parametrize("name", [n for n in mtf.CASES if n.startswith("vga")])
def test_reference_fixture_cases(name):
    gold = np.load(mtf.OUT)
    _, _, net_in, net_out, mode, _, _ = mtf.CASES[name]
    got = image_proc.training_batch_from_frames(mtf.frames(name), mtf.keypoints(name), net_in, net_out, mode, MEAN, STDEV)
    assert np.array_equal(got["keypoint_projections_input"].cpu().numpy(), gold[name + ".netin"])
    assert np.array_equal(got["keypoint_projections_output"].cpu().numpy(), gold[name + ".netout32"])
    assert np.array_equal(got["belief_maps"].cpu().numpy(), gold[name + ".belief_maps"])


@pytest.mark.parametrize("w,h,net_in,net_out", [(640, 480, (400, 400), (100, 100)), (1280, 720, (400, 400), (100, 100)),
                                                (1920, 1080, (208, 208), (52, 52))])
def test_augmentation_matches_restatement(w, h, net_in, net_out):
    mode, b = "shrink-and-crop", 8
    frames, kps = raw_batch(b, w, h, seed=1)
    table = mixed_table(b, net_in)
    got = image_proc.training_batch_from_frames(torch.from_numpy(frames).cuda(), kps, net_in, net_out, mode, MEAN, STDEV,
                                                augmentation=table, return_u8=True)
    resized = mfp.pil_preprocess(frames, net_in, mode)
    want = restated_batch(resized, table)
    assert np.array_equal(got["image_rgb_input_u8"].cpu().numpy(), want)
    assert torch.equal(got["image_rgb_input"].cpu(), host_input(want))
    netin, netout = restated_keypoints(kps, table, (w, h), net_in, net_out, mode)
    assert np.array_equal(got["keypoint_projections_input"].cpu().numpy(), netin)
    assert np.array_equal(got["keypoint_projections_output"].cpu().numpy(), netout)
    assert np.array_equal(got["belief_maps"].cpu().numpy(), host_belief_maps(netout, net_out))
    plain = image_proc.training_batch_from_frames(frames, kps, net_in, net_out, mode, MEAN, STDEV)
    assert torch.equal(plain["image_rgb_input"][0], got["image_rgb_input"][0])            # row 0 is off
    assert not torch.equal(plain["image_rgb_input"], got["image_rgb_input"])              # the feature is not a no-op
    assert not torch.equal(plain["belief_maps"], got["belief_maps"])
    off = image_proc.training_batch_from_frames(frames, kps, net_in, net_out, mode, MEAN, STDEV,
                                                augmentation=image_proc.AugmentationTable(b))
    for key in plain:
        assert torch.equal(plain[key], off[key]), key


def test_batch128_each_frame_equals_the_frame_alone():
    net_in, net_out, mode, b = (400, 400), (100, 100), "shrink-and-crop", 128
    frames, kps = raw_batch(b, 640, 480, seed=2)
    table = image_proc.sample_augmentation(b, net_in, np.random.RandomState(7))
    f = torch.from_numpy(frames).cuda()
    got = image_proc.training_batch_from_frames(f, kps, net_in, net_out, mode, MEAN, STDEV, augmentation=table)
    again = image_proc.training_batch_from_frames(f, kps, net_in, net_out, mode, MEAN, STDEV, augmentation=table)
    for key in got:
        assert torch.equal(got[key], again[key]), key
    for i in range(b):
        one = image_proc.training_batch_from_frames(f[i:i + 1], kps[i:i + 1], net_in, net_out, mode, MEAN, STDEV,
                                                    augmentation=table.row(i))
        for key in got:
            assert torch.equal(one[key][0], got[key][i]), (key, i)


def test_shifted_blob_moves_with_its_keypoint():
    net_in, net_out, mode = (400, 400), (100, 100), "shrink-and-crop"
    frames, _ = raw_batch(1, 640, 480, seed=3)
    kps = np.array([[[320.0, 240.0], [200.5, 100.25]]])
    shift = image_proc.AugmentationTable(1, matrix=[[[1.0, 0.0, 10.0], [0.0, 1.0, 0.0]]])
    plain = image_proc.training_batch_from_frames(frames, kps, net_in, net_out, mode, MEAN, STDEV)
    moved = image_proc.training_batch_from_frames(frames, kps, net_in, net_out, mode, MEAN, STDEV, augmentation=shift)
    assert np.array_equal(moved["keypoint_projections_input"].cpu().numpy(), plain["keypoint_projections_input"].cpu().numpy() + [10.0, 0.0])
    for j in range(2):
        x, y = moved["keypoint_projections_output"][0, j].tolist()
        m = moved["belief_maps"][0, j]
        assert m.max().item() == 1.0 and m[int(y), int(x)].item() == 1.0
        px = plain["keypoint_projections_output"][0, j, 0].item()
        assert int(x) != int(px) and plain["belief_maps"][0, j][int(y), int(px)].item() == 1.0


def twin_networks():
    import cases
    import parity_checks as pc
    from oracle import models as om
    nets = []
    for _ in range(2):
        wts = om.recipe_weights(om.build_model("vgg_q", 7).state_dict(), cases.TRAIN_FINAL_KEYS, cases.TRAIN_FINAL_SCALE)
        net = pc.build_network("vgg_q", "cuda", weights=wts, optimizer="adam", lr=1e-5, in_res=(200, 200))
        net.enable_training()
        nets.append(net)
    return nets


@pytest.mark.parametrize("graph", [False, True])
def test_train_from_frames_equals_train_on_a_host_built_batch(graph):
    from PIL import Image
    a, b = twin_networks()
    a.hip_graph_train = b.hip_graph_train = graph
    frames, kps = raw_batch(4, 400, 300, seed=4)
    net_in, net_out, mode = a.trained_net_input_resolution(), a.trained_net_output_resolution(), a.image_preprocessing()
    norm = a.image_normalization
    pil = np.stack([np.asarray(image_proc.preprocess_image(Image.fromarray(f), net_in, mode)) for f in frames])
    x = torch.from_numpy(np.ascontiguousarray(((pil.astype(np.float32) / np.float32(255.0) - np.asarray(norm["mean"], np.float32))
                                               / np.asarray(norm["stdev"], np.float32)).transpose(0, 3, 1, 2)))
    target = []
    for k in kps:
        k_in = image_proc.convert_keypoints_to_netin_from_raw(k, (400, 300), net_in, mode)
        k_out = torch.from_numpy(image_proc.convert_keypoints_to_netout_from_netin(k_in, net_in, net_out)).float()
        target.append(torch.tensor(image_proc.create_belief_map(net_out, k_out)).float())
    target = torch.stack(target)
    assert a.loss_from_frames(frames, kps).item() == b.loss([x], target).item()
    for _ in range(2):
        assert a.train_from_frames(frames, kps).item() == b.train([x], target).item()
    for (key, p), (_, q) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
        assert torch.equal(p, q), key
    # with an augmentation table: equal to train() on the batch training_batch_from_frames returns for it
    table = image_proc.sample_augmentation(4, net_in, np.random.RandomState(8), p=1.0)
    batch = image_proc.training_batch_from_frames(frames, kps, net_in, net_out, mode, norm["mean"], norm["stdev"], augmentation=table)
    assert a.train_from_frames(torch.from_numpy(frames).cuda(), kps, augmentation=table).item() == \
        b.train([batch["image_rgb_input"]], batch["belief_maps"]).item()
    for (key, p), (_, q) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
        assert torch.equal(p, q), key
    with pytest.raises(AssertionError):
        a.train_from_frames(frames, kps, image_preprocessing_override="shrink")       # 266 x 200 is not the trained resolution
