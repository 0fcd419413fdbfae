"""CPU: the torch restatement of LPIPS-alex (tests/lpips_ref.py) at hand values, and the host side of the product's
weight handling (tta/lpips.py: both file layouts, named errors, the synthetic draw, the environment switch)."""
import pytest
import torch

import lpips_ref as R


def _sd(seed=0):
    return R.synthetic_state_dict(seed)


def test_identical_inputs_score_exactly_zero():
    gen, gt_u8 = R.frames(2, 40, 52, seed=1)
    for dtype in (torch.float64, torch.float32):
        assert torch.equal(R.lpips(gen, gen.clone(), _sd(), dtype), torch.zeros(2, dtype=dtype))
        # a uint8 ground truth against its own fp32 image: the same values after / 255
        assert torch.equal(R.lpips(gt_u8.float() / 255.0, gt_u8, _sd(), dtype), torch.zeros(2, dtype=dtype))


def test_one_hot_features_give_the_lin_weight():
    """One pixel, generated feature e_a, ground truth e_b (a != b): the normalised difference is +1 at a and -1 at b,
    so the tap distance is w_a + w_b; against a zero feature (which normalises to zero) it is w_a alone."""
    C = 64
    w = torch.rand(C, dtype=torch.float64)
    fa, fb = torch.zeros(1, C, 1, 1, dtype=torch.float64), torch.zeros(1, C, 1, 1, dtype=torch.float64)
    fa[0, 5], fb[0, 9] = 3.0, 0.25                      # the magnitudes normalise away
    assert R.tap_distance(fa, fb, w).item() == pytest.approx((w[5] + w[9]).item(), rel=1e-9)
    assert R.tap_distance(fa, torch.zeros_like(fa), w).item() == pytest.approx(w[5].item(), rel=1e-9)
    # spatial mean: the same pair on one of four pixels
    fa4, fb4 = torch.zeros(1, C, 2, 2, dtype=torch.float64), torch.zeros(1, C, 2, 2, dtype=torch.float64)
    fa4[0, 5, 1, 0] = 1.0
    assert R.tap_distance(fa4, fb4, w).item() == pytest.approx(w[5].item() / 4, rel=1e-9)


def test_tap_sizes_and_smallest_frame():
    sd = _sd()
    shapes = [tuple(t.shape) for t in R.taps(torch.zeros(1, 480, 832, 3), sd, torch.float32)]
    assert shapes == [(1, 64, 119, 207), (1, 192, 59, 103), (1, 384, 29, 51), (1, 256, 29, 51), (1, 256, 29, 51)]
    assert [tuple(t.shape[2:]) for t in R.taps(torch.zeros(1, 31, 31, 3), sd, torch.float32)] == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    with pytest.raises(ValueError, match="smaller than 31x31"):
        R.lpips(torch.zeros(1, 30, 40, 3), torch.zeros(1, 30, 40, 3), sd)


def test_scaling_layer_and_symmetry():
    x = R.scale_input(torch.full((1, 2, 2, 3), 0.5), torch.float64)      # 2 * 0.5 - 1 = 0 -> -shift / scale
    want = torch.tensor([0.030 / 0.458, 0.088 / 0.448, 0.188 / 0.450], dtype=torch.float64)
    assert torch.allclose(x[0, :, 0, 0], want, rtol=1e-7)
    gen, gt_u8 = R.frames(2, 37, 45, seed=2, noise=0.3)
    gt = gt_u8.float() / 255.0
    a, b = R.lpips(gen, gt, _sd()), R.lpips(gt, gen, _sd())
    assert torch.equal(a, b) and (a > 1e-4).all() and (a < 2).all()
    # the fp32 evaluation of the same network agrees with float64 to fp32 rounding
    a32 = R.lpips(gen, gt, _sd(), torch.float32).double()
    assert ((a32 - a).abs() / a).max() < 5e-6
    # more noise, more distance
    gen_lo, _ = R.frames(2, 37, 45, seed=2, noise=0.08)
    assert (R.lpips(gen_lo, gt, _sd()) < a).all()


def test_product_synthetic_draw_is_the_documented_one():
    from tta.lpips import LpipsAlex
    mine, theirs = _sd(7), LpipsAlex.synthetic_state_dict(7)
    assert set(mine) == set(theirs) and all(torch.equal(mine[k], theirs[k]) for k in mine)
    assert all((theirs[f"lin{i}.model.1.weight"] >= 0).all() for i in range(5))
    assert not torch.equal(LpipsAlex.synthetic_state_dict(8)["lin0.model.1.weight"], theirs["lin0.model.1.weight"])


def test_weight_loader_round_trips_both_layouts_and_names_what_is_missing(tmp_path):
    from tta import lpips as L
    sd = _sd(3)
    sd["scaling_layer.shift"] = torch.tensor(R.SHIFT).view(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(R.SCALE).view(1, 3, 1, 1)
    one = tmp_path / "lpips_alex.pt"
    torch.save(sd, one)
    got, source = L.read_state_dict(one)
    assert source == str(one) and set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    # torchvision's file (with its classifier and pools' worth of other keys) + the package's lin file
    tv = {f"features.{j}.{leaf}": sd[f"net.slice{i + 1}.{j}.{leaf}"] for i, j in enumerate((0, 3, 6, 8, 10)) for leaf in ("weight", "bias")}
    tv["classifier.1.weight"] = torch.zeros(4, 4)
    lin = {f"lin{i}.model.1.weight": sd[f"lin{i}.model.1.weight"] for i in range(5)}
    d = tmp_path / "pair"
    d.mkdir()
    torch.save(tv, d / "alexnet-owt-7be5be79.pth")
    torch.save(lin, d / "alex.pth")
    for got, _ in (L.read_state_dict(d), L.read_state_dict(d / "alexnet-owt-7be5be79.pth", d / "alex.pth")):
        assert all(torch.equal(got[k], sd[k]) for k in sd if not k.startswith("scaling_layer")) and "scaling_layer.shift" not in got
    # errors name the key
    broken = dict(sd); del broken["net.slice3.6.bias"]
    torch.save(broken, one)
    with pytest.raises(KeyError, match=r"net\.slice3\.6\.bias"):
        L.read_state_dict(one)
    wrong = dict(sd); wrong["lin2.model.1.weight"] = torch.zeros(1, 256, 1, 1)
    torch.save(wrong, one)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight.*\(1, 384, 1, 1\)"):
        L.read_state_dict(one)
    del lin["lin4.model.1.weight"]
    torch.save(lin, d / "alex.pth")
    with pytest.raises(KeyError, match=r"lin4\.model\.1\.weight"):
        L.read_state_dict(d)
    torch.save(tv, one)                                    # a bare torchvision file is not enough
    with pytest.raises(KeyError, match=r"net\.slice1\.0\.weight"):
        L.read_state_dict(one)
    with pytest.raises(FileNotFoundError, match="alex.pth"):
        L.read_state_dict(tmp_path)


def test_environment_switch_defaults_to_no_model(monkeypatch):
    from tta import lpips as L
    monkeypatch.delenv(L.ENV_VAR, raising=False)
    assert L.model_from_env() is None
    monkeypatch.setenv(L.ENV_VAR, "  ")
    assert L.model_from_env() is None
    assert L.ENV_VAR == "LCV_LPIPS_WEIGHTS"


def test_ops_refuse_the_cpu_and_small_frames():
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    with pytest.raises(LcvError, match="GPU"):
        ops.lpips_alex(torch.zeros(1, 40, 40, 3), torch.zeros(1, 40, 40, 3), None)
    with pytest.raises(LcvError, match="GPU"):
        ops.lpips_pack_weight(torch.zeros(64, 3, 11, 11))
