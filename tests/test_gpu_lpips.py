"""GPU parity of the on-device LPIPS-alex (csrc/lpips.hip, include/lcv_hip_lpips.h) against the float64 torch
restatement in tests/lpips_ref.py: each kernel on its own, then `ops.lpips_alex` end to end, then the public path
(`evaluate_generation_metrics`, two runners).

Bounds.
* Convolution kernels, against float64 `F.conv2d` + ReLU: every output within 1e-6 * (sum_k |x_k w_k| + |bias|) and the
  whole map within 1e-6 relative L2.  Reasoning: the f32-input MFMA is a k-ordered fp32 fma chain (0.75e-7 ... 1.5e-7 of
  sum |ab| for a whole chain at K <= 1024); the kernel restarts the chain every 32 k (expected u sqrt(32) / 2.4 =
  1.4e-7 relative) and adds the chunk sums with compensation, so 1e-6 is about seven standard deviations - room for the
  maximum over 1e5 outputs, none for a wrong tap or a dropped chunk (one product missing of K is >= 3e-4).
* Tap distance on independent random halves (no cancellation between them): 1e-6 relative, about eight fp32 roundings
  per term.
* End to end, as the issue sets it: relative to the float64 restatement, err_kernel <= 4 * max(err_fp32_cpu, 2.5e-7),
  where err_fp32_cpu is the deviation of the fp32 `F.conv2d` evaluation of the same network on the same inputs.
  Measured on one MI355X (err_kernel / err_fp32_cpu, relative; the table is in profiles/r06_lpips.md):
  31x31 N=1 u8 1.03e-7 / 1.19e-8; 31x31 N=3 fp32 8.18e-8 / 2.00e-7; 37x101 N=3 fp32 3.18e-8 / 1.02e-7;
  37x101 N=1 u8 6.85e-8 / 6.85e-8; 45x96 N=3 u8 7.06e-8 / 1.18e-7; 45x96 N=1 fp32 2.07e-8 / 9.81e-8;
  64x342 N=1 u8 5.20e-8 / 4.72e-8; 64x342 N=3 fp32 2.44e-8 / 1.05e-7; 480x832 u8 1.45e-8 / 1.45e-8;
  720x1280 fp32 8.64e-8 / 2.62e-8.  The bound is never below 1e-6; nothing needs a tenth of it.
* Identical frames score exactly 0.0: both halves of a pair go through the same instructions on the same values.
  Swapped arguments are equal to the last bit: a generated frame and a ground-truth frame take the same path through
  every kernel (each output element's sum order does not depend on where the image sits in the batch), and
  (a - b)^2 == (b - a)^2 in IEEE arithmetic.
"""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def model():
    from tta.lpips import LpipsAlex
    return LpipsAlex.synthetic(0)


SD = R.synthetic_state_dict(0)


def _nhwc(t):      # NCHW -> channels-last contiguous
    return t.permute(0, 2, 3, 1).contiguous()


def test_pack_weight_layout():
    from lcv_hip import ops
    for cout, cin, k in ((64, 3, 11), (192, 64, 5), (128, 32, 3)):
        w = torch.randn(cout, cin, k, k, generator=torch.Generator().manual_seed(cout))
        got = ops.lpips_pack_weight(w.cuda()).cpu()
        K = k * k * cin
        assert got.shape == (cout, (K + 31) // 32 * 32)
        assert torch.equal(got[:, :K], w.permute(0, 2, 3, 1).reshape(cout, K))      # (kh, kw, ci), ci fastest
        assert torch.equal(got[:, K:], torch.zeros(cout, got.shape[1] - K))


@pytest.mark.parametrize("layer,B,h,w", [(1, 2, 13, 17), (2, 2, 7, 9), (3, 4, 7, 9), (4, 2, 29, 51), (1, 1, 3, 3)])
def test_conv_relu_layers_match_float64_conv2d(layer, B, h, w):
    """Layers 2-5 on channels-last inputs whose M is not a multiple of the 128-pixel tile (and one smaller than a wave)."""
    from lcv_hip import ops
    key, cin, cout, k, stride, pad, _ = R.LAYERS[layer]
    g = torch.Generator().manual_seed(100 * layer + h)
    x = torch.relu(torch.randn(B, cin, h, w, generator=g))                      # what a previous ReLU hands over
    wt, b = SD[key + ".weight"], SD[key + ".bias"]
    got = ops.lpips_conv_relu(_nhwc(x).cuda(), ops.lpips_pack_weight(wt.cuda()), b.cuda(), k, stride, pad).cpu()
    ref = F.relu(F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=pad))
    mag = F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs(), stride=stride, padding=pad)
    assert got.shape == _nhwc(ref).shape
    err = (got.double() - _nhwc(ref)).abs() / _nhwc(mag)
    rel = (torch.linalg.vector_norm(got.double() - _nhwc(ref)) / torch.linalg.vector_norm(ref)).item()
    print(f"conv layer {layer + 1} B={B} {h}x{w}: max err / sum|ab| = {err.max().item():.3g}, rel L2 = {rel:.3g}")
    assert err.max().item() <= 1e-6 and rel <= 1e-6


@pytest.mark.parametrize("N,H,W,u8", [(1, 31, 31, True), (2, 45, 96, False), (1, 64, 342, True)])
def test_first_layer_scales_the_frames_in_its_loader(N, H, W, u8, model):
    """conv1 straight from the [N,H,W,3] frames: 2x - 1, the scaling layer, zero padding after it, uint8 / 255."""
    from lcv_hip import ops
    gen, gt_u8 = R.frames(N, H, W, seed=H + W)
    gt = gt_u8 if u8 else gt_u8.float() / 255.0
    got = ops.lpips_conv1_relu(gen.cuda(), gt.cuda(), model.weights).cpu()
    key, _, _, k, stride, pad, _ = R.LAYERS[0]
    x = torch.cat([R.scale_input(gen, torch.float64), R.scale_input(gt, torch.float64)])
    wt, b = SD[key + ".weight"].double(), SD[key + ".bias"].double()
    ref = _nhwc(F.relu(F.conv2d(x, wt, b, stride=stride, padding=pad)))
    mag = _nhwc(F.conv2d(x.abs(), wt.abs(), b.abs(), stride=stride, padding=pad))
    assert got.shape == ref.shape
    err = ((got.double() - ref).abs() / mag).max().item()
    rel = (torch.linalg.vector_norm(got.double() - ref) / torch.linalg.vector_norm(ref)).item()
    print(f"conv1 N={N} {H}x{W} u8={u8}: max err / sum|ab| = {err:.3g}, rel L2 = {rel:.3g}")
    assert err <= 1e-6 and rel <= 1e-6


@pytest.mark.parametrize("B,h,w,C", [(2, 7, 7, 64), (3, 14, 25, 192), (1, 3, 3, 64), (2, 8, 11, 256)])
def test_maxpool_is_exact(B, h, w, C):
    from lcv_hip import ops
    x = torch.randn(B, C, h, w, generator=torch.Generator().manual_seed(h * w))
    got = ops.lpips_maxpool(_nhwc(x).cuda()).cpu()
    assert torch.equal(got, _nhwc(F.max_pool2d(x, kernel_size=3, stride=2)))


@pytest.mark.parametrize("N,h,w,C", [(1, 1, 1, 256), (3, 7, 7, 64), (2, 13, 17, 192), (2, 29, 51, 384), (1, 40, 41, 256)])
def test_tap_distance_matches_restatement(N, h, w, C):
    from lcv_hip import ops
    g = torch.Generator().manual_seed(C + h)
    f = torch.relu(torch.randn(2 * N, C, h, w, generator=g))
    f[0, :, 0, 0] = 0.0                                        # an all-zero feature normalises to zero (0 / 1e-10), not NaN
    lin = torch.rand(C, generator=g) * (2.0 / C)
    ref = R.tap_distance(f[:N].double(), f[N:].double(), lin.double())
    fd = _nhwc(f).cuda()
    out = ops.lpips_tap_distance(fd, lin.cuda())
    rel = ((out.cpu().double() - ref).abs() / ref).max().item()
    print(f"tap distance N={N} {h}x{w}x{C}: rel err = {rel:.3g}")
    assert rel <= 1e-6
    twice = ops.lpips_tap_distance(fd, lin.cuda(), out=out.clone(), accumulate=True)
    assert torch.equal(twice, out + out)                       # accumulate adds the same mean; fixed-order partial sums
    assert torch.equal(ops.lpips_tap_distance(fd, lin.cuda()), out)


def _check_end_to_end(model, N, H, W, u8, noise, seed):
    from lcv_hip import ops
    gen, gt_u8 = R.frames(N, H, W, seed=seed, noise=noise)
    gt = gt_u8 if u8 else gt_u8.float() / 255.0
    ref64 = R.lpips(gen, gt, SD, torch.float64)
    ref32 = R.lpips(gen, gt, SD, torch.float32).double()
    gd, td = gen.cuda(), gt.cuda()
    out = ops.lpips_alex(gd, td, model.weights)
    assert out.shape == (N,) and out.dtype == torch.float32 and out.is_cuda
    err_cpu = ((ref32 - ref64).abs() / ref64).max().item()
    err_kernel = ((out.cpu().double() - ref64).abs() / ref64).max().item()
    print(f"lpips_alex N={N} {H}x{W} u8={u8} noise={noise}: lpips={ref64.mean().item():.4g} "
          f"err_kernel={err_kernel:.3g} err_fp32_cpu={err_cpu:.3g}")
    assert (ref64 > 1e-4).all()                                 # not a degenerate case
    assert err_kernel <= 4 * max(err_cpu, 2.5e-7)
    assert torch.equal(ops.lpips_alex(gd, td, model.weights), out)              # two runs, the same bits
    return gd, td, out


@pytest.mark.parametrize("N,H,W,u8,noise", [(1, 31, 31, True, 0.08), (3, 31, 31, False, 0.3), (3, 37, 101, False, 0.08),
                                            (1, 37, 101, True, 0.3), (3, 45, 96, True, 0.08), (1, 45, 96, False, 0.3),
                                            (1, 64, 342, True, 0.08), (3, 64, 342, False, 0.3)])
def test_lpips_alex_matches_float64_restatement(N, H, W, u8, noise, model):
    from lcv_hip import ops
    gd, td, out = _check_end_to_end(model, N, H, W, u8, noise, seed=H * W + N)
    # the fp32 image of a uint8 frame is taken on the host: a true division, the correctly rounded quotient the kernels'
    # loader produces (the device's `tensor / 255.0` multiplies by a rounded reciprocal and is 1 ulp off on some values)
    gt_f = (td.cpu().float() / 255.0).cuda() if u8 else td
    assert torch.equal(ops.lpips_alex(gt_f, td, model.weights), torch.zeros(N, device="cuda"))    # identical frames: exactly 0.0
    assert torch.equal(ops.lpips_alex(gt_f, gd, model.weights), ops.lpips_alex(gd, gt_f, model.weights))   # swapped: last bit
    one = ops.lpips_alex(gd[N - 1:], td[N - 1:], model.weights)
    assert one[0] == out[N - 1]                                 # a pair's value does not depend on its batch


def test_lpips_alex_480p_pair(model):
    from lcv_hip import ops
    gd, td, out = _check_end_to_end(model, 1, 480, 832, True, 0.08, seed=3)
    gt_f = (td.cpu().float() / 255.0).cuda()                    # host division: see the note in the test above
    assert ops.lpips_alex(gt_f, td, model.weights)[0].item() == 0.0
    assert torch.equal(ops.lpips_alex(gt_f, gd, model.weights), ops.lpips_alex(gd, gt_f, model.weights))


def test_lpips_alex_720p_pair(model):
    _check_end_to_end(model, 1, 720, 1280, False, 0.3, seed=4)


def test_more_pairs_than_one_pass(model):
    """N above the pairs-per-pass of ops.lpips_alex: the passes share one workspace and every pair keeps its value."""
    from lcv_hip import ops
    N = ops.LPIPS_CHUNK + 3
    gen, gt_u8 = R.frames(N, 40, 52, seed=9, noise=0.3)
    out = ops.lpips_alex(gen.cuda(), gt_u8.cuda(), model.weights)
    ref = R.lpips(gen, gt_u8, SD, torch.float64)
    assert ((out.cpu().double() - ref).abs() / ref).max().item() <= 1e-6
    for i in (0, ops.LPIPS_CHUNK - 1, ops.LPIPS_CHUNK, N - 1):
        assert ops.lpips_alex(gen[i:i + 1].cuda(), gt_u8[i:i + 1].cuda(), model.weights)[0] == out[i]


def test_rejects_bad_arguments(model):
    from lcv_hip import ops
    from lcv_hip.lib import LcvError, call
    g = torch.zeros(1, 30, 40, 3, device="cuda")
    with pytest.raises(LcvError, match="smaller than 31x31"):
        ops.lpips_alex(g, g, model.weights)
    with pytest.raises(LcvError, match="equal shape"):
        ops.lpips_alex(torch.zeros(1, 40, 40, 3, device="cuda"), torch.zeros(1, 40, 44, 3, device="cuda"), model.weights)
    with pytest.raises(LcvError, match="equal shape"):
        ops.lpips_alex(torch.zeros(1, 40, 40, 4, device="cuda"), torch.zeros(1, 40, 40, 4, device="cuda"), model.weights)
    with pytest.raises(LcvError, match="GPU"):
        ops.lpips_alex(torch.zeros(1, 40, 40, 3), torch.zeros(1, 40, 40, 3), model.weights)
    with pytest.raises(LcvError, match="fp32 or uint8"):
        ops.lpips_alex(torch.zeros(1, 40, 40, 3, device="cuda"), torch.zeros(1, 40, 40, 3, device="cuda", dtype=torch.float16), model.weights)
    with pytest.raises(LcvError, match="LpipsWeights"):
        ops.lpips_alex(torch.zeros(1, 40, 40, 3, device="cuda"), torch.zeros(1, 40, 40, 3, device="cuda"), None)
    # the C ABI itself refuses what the second pool cannot window, with LCV_EINVAL and a message
    x = torch.zeros(2, 2, 2, 192, device="cuda")
    with pytest.raises(LcvError, match="smaller than the 3x3 window") as e:
        call("lcv_lpips_maxpool", x.data_ptr(), x.data_ptr(), 2, 2, 2, 192, None)
    assert e.value.code == -1


def test_evaluate_generation_metrics_fills_lpips(model):
    from tta.eval_metrics import evaluate_generation_metrics
    gen, gt_u8 = R.frames(3, 48, 64, seed=11, noise=0.3)
    full = torch.cat([torch.zeros(2, *gen.shape[1:]), gen, torch.ones(1, *gen.shape[1:])]).cuda()
    want = float(R.lpips(gen, gt_u8, SD).mean())
    for flavour in ("tta", "baseline"):
        m = evaluate_generation_metrics(full, gt_u8.cuda(), 2, 3, flavour=flavour, lpips_model=model)
        assert abs(m["lpips"] - want) <= 1e-6 * want and m["psnr"] > 0
    m2 = evaluate_generation_metrics(full, gt_u8[:2].cuda(), 2, 3, lpips_model=model)        # n_compare = min(gen, gt)
    assert abs(m2["lpips"] - float(R.lpips(gen[:2], gt_u8[:2], SD).mean())) <= 1e-6 * want
    m3 = evaluate_generation_metrics(full, gt_u8.cuda(), 2, 3)
    assert m3["lpips"] != m3["lpips"]                                                         # opt-in: NaN without a model
    e = evaluate_generation_metrics(full[:2], gt_u8.cuda(), 2, 3, lpips_model=model)
    assert all(v != v for v in e.values())


def _run(rel, argv):
    path = ROOT / "longcat-video-tta_amd" / rel
    spec = importlib.util.spec_from_file_location("lpips_runner_" + path.stem, path)
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    m.main(argv)


def test_lora_runner_rows_carry_lpips_when_weights_are_named(tmp_path, monkeypatch):
    argv = ["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:2", "--num-cond-frames", "5", "--num-frames", "13",
            "--gen-start-frame", "40", "--tta-total-frames", "33", "--tta-context-frames", "9", "--num-steps", "2", "--es-disable",
            "--num-inference-steps", "2", "--lora-rank", "4", "--lora-alpha", "8", "--no-save-videos"]
    monkeypatch.setenv("LCV_LPIPS_WEIGHTS", "synthetic:0")
    _run("lora_experiment/scripts/run_lora_tta.py", argv + ["--output-dir", str(tmp_path / "with")])
    s = json.loads((tmp_path / "with" / "summary.json").read_text())
    assert s["num_successful"] == 2
    vals = [r["lpips"] for r in s["results"]]
    assert all(isinstance(v, float) and np.isfinite(v) and 0 < v < 2 for v in vals), vals
    assert s["lpips"] == pytest.approx(sum(vals) / 2, abs=1e-6) and all(r["psnr"] > 0 for r in s["results"])
    monkeypatch.delenv("LCV_LPIPS_WEIGHTS")
    _run("lora_experiment/scripts/run_lora_tta.py", argv + ["--output-dir", str(tmp_path / "without")])
    s = json.loads((tmp_path / "without" / "summary.json").read_text())
    assert s["num_successful"] == 2 and s["lpips"] is None and all(r["lpips"] is None for r in s["results"])


def test_baseline_runner_fills_lpips_stats(tmp_path, monkeypatch):
    monkeypatch.setenv("LCV_LPIPS_WEIGHTS", "synthetic:0")
    out = tmp_path / "base"
    _run("baseline_experiment/scripts/run_baseline.py",
         ["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:2", "--output-dir", str(out), "--num-cond-frames", "5",
          "--num-gen-frames", "8", "--num-inference-steps", "2"])
    s = json.loads((out / "summary.json").read_text())
    st = s["metrics"]["lpips"]
    assert set(st) == {"mean", "std", "min", "max"} and 0 < st["min"] <= st["mean"] <= st["max"] < 2
    assert st["mean"] == round(st["mean"], 4)                  # 4 decimals, as the reference's baseline row
    rows = (out / "per_video_metrics.csv").read_text().splitlines()
    assert rows[0].split(",")[5] == "lpips" and all(0 < float(r.split(",")[5]) < 2 for r in rows[1:])
