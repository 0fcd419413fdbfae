"""Every VAE convolution kernel against tests/conv_ref.py, BIT FOR BIT, at batch, border and tile edges.

Small-integer data (x in [-3, 3], w in [-2, 2], bias and residual in [-8, 8]) makes every bf16 x bf16 product and every fp32
partial sum an exact integer below 2^17, so the result does not depend on the summation order and the only rounding is the
RNE store to bf16: each kernel behind lcv_causal_conv3d / lcv_conv3d_strided - conv16_igemm<128x128>, <256x256>, <256x192>,
<192x192x3>, conv_wide<256x192>, conv8p_igemm<256x256>, conv_rows<256x96>, <256x16> - must give bf16(float64 convolution) in
every pixel and channel (tests/test_conv_ref.py holds the argument).  One wrong tap at one border pixel fails here; under the
aggregate bounds of tests/test_gpu_vae.py it does not.

Each test computes its float64 reference once and runs it over the knob settings, with and without a residual; after every
run the kernel the library reports (lcv_conv3d_last_kernel) is compared with the one the setting must select.
"""
import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

_VAE = []


def _vae():
    if not _VAE:
        from longcat_video.modules.vae_wan import AutoencoderKLWan
        _VAE.append(AutoencoderKLWan(base_dim=16, z_dim=4, device="cuda", dtype=BF16))
    return _VAE[0]


def _last_kernel():
    from lcv_hip import lib
    return lib.load().lcv_conv3d_last_kernel().decode()


def _module(w, bias):
    """The product's parameter holder with the reference's integer weights: the kernel weight comes from `_Conv.packed()`."""
    from longcat_video.modules.vae_wan import _Conv
    co, ci, kt, kh, kw = w.shape
    k = (kh, kw) if kt == 1 and (kh, kw) != (1, 1) else (kt, kh, kw)
    conv = _Conv(ci, co, k, device="cuda", dtype=BF16)
    with torch.no_grad():
        conv.weight.copy_(w.view(conv.weight.shape))
        conv.bias.copy_(bias)
    assert torch.equal(conv.packed().cpu(), R.pack_weight(w))
    return conv


def _assert_exact(got, want, cout, knobs):
    """torch.equal over the whole channels-last tensor, padding channels included; a mismatch names the kernel, the knobs, the
    number of differing elements and the first (b, t, h, w, c) coordinates."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == BF16
    if not torch.equal(got, want):
        bad = (got.float() != want.float()) | got.float().isnan()
        where = bad.nonzero()[:6].tolist()
        pairs = [(tuple(i), got[tuple(i)].item(), want[tuple(i)].item()) for i in where]
        raise AssertionError(f"{_last_kernel()} under {knobs or 'default knobs'}: {int(bad.sum())} of {bad.numel()} elements differ "
                             f"(shape {tuple(got.shape)}, Cout {cout}); first (b,t,h,w,c), got, want: {pairs}")
    assert got.shape[-1] == cout or float(got[..., cout:].float().abs().max()) == 0, f"{_last_kernel()}: padding channels not zero"


def _run_settings(run, wants, cout, settings, monkeypatch):
    """`run(resid_key)` launches once; every knob setting x {no residual, residual} must reproduce `wants[resid_key]`."""
    for env, name in settings:
        for kname, v in env.items():
            monkeypatch.setenv(kname, v)
        for key in (False, True):
            got = run(key)
            assert _last_kernel() == name, (env, _last_kernel(), name)
            _assert_exact(got, wants[key], cout, dict(env, resid=key))
        for kname in env:
            monkeypatch.delenv(kname)


def _causal_case(B, T, Hin, Win, ci, co, k, up, seed):
    """Data, module and both expected outputs (kernel layout) of one causal convolution; Cout = 3 is the unpadded head."""
    x, w = R.make_x(B, ci, T, Hin, Win, seed), R.make_w(co, ci, k, seed + 1)
    bias = R.make_bias(co, seed + 2)
    H, W = (2 * Hin, 2 * Win) if up else (Hin, Win)
    resid = R.make_resid(B, co, T, H, W, seed + 3)
    R.check_data_rules(x, w, bias, resid)
    acc = R.causal_conv3d(x, w, up2x=up)
    pad_out = co != 3
    wants = {False: R.to_kernel_layout(R.finish(acc, bias), pad_out), True: R.to_kernel_layout(R.finish(acc, bias, resid), pad_out)}
    assert not torch.equal(wants[False], wants[True]) and float(wants[False].float().abs().max()) > 0
    conv, xc, rc = _module(w, bias), R.to_kernel_layout(x).cuda(), R.to_kernel_layout(resid, pad_out).cuda()
    run = lambda with_resid: _vae()._conv(xc, conv, resid=rc if with_resid else None, up2x=up, pad_out=pad_out)
    return run, wants


# ---------------------------------------------------------------------------------------------------------------------------
# causal stride-1 form, implicit-GEMM family
# ---------------------------------------------------------------------------------------------------------------------------
_DEFAULT_128 = [({}, "conv16_igemm<128x128>")]
_WIDE_192 = [({}, "conv_wide<256x192>"), ({"LCV_CONV_N192": "2"}, "conv16_igemm<256x192>"),
             ({"LCV_CONV_N192": "3"}, "conv16_igemm<192x192x3>"), ({"LCV_CONV_N192": "0"}, "conv16_igemm<256x256>"),
             ({"LCV_CONV_8P": "1"}, "conv8p_igemm<256x256>")]
_WIDE_256 = [({}, "conv16_igemm<256x256>"), ({"LCV_CONV_8P": "1"}, "conv8p_igemm<256x256>")]
_IGEMM_CHANNELS = [
    (32, 64, _DEFAULT_128),      # ldx = 64 with 32 zero padding channels
    (64, 3, _DEFAULT_128),       # pad_out=False: ldc = 3
    (160, 96, _DEFAULT_128),     # ldx = 192; 128x128 tile with N partial
    (64, 192, _WIDE_192),        # one 192-column tile
    (192, 384, _WIDE_192),       # two 192-column tiles
    (64, 320, _WIDE_256),        # 256x256 tile with a partial second column tile
]
_K333, _K33, _K33UP, _K311, _K111 = ((3, 3, 3), False), ((3, 3), False), ((3, 3), True), ((3, 1, 1), False), ((1, 1, 1), False)
_IGEMM_GEOMETRIES = [
    # B, T, H, W (input), kernels
    ((2, 3, 5, 7), (_K333, _K33, _K33UP, _K311, _K111)),   # M = 210: one partial tile holding the batch boundary, nearly all border
    ((3, 1, 1, 1), (_K333, _K33UP)),                       # M = 3: only the last temporal and the centre spatial tap are valid
    ((2, 2, 9, 31), (_K333, _K33UP)),                      # M = 1116: tile edges inside a row, a frame and the batch
]
_IGEMM_CASES = [(g, k, up, ci, co, s) for g, ks in _IGEMM_GEOMETRIES for (k, up) in ks for (ci, co, s) in _IGEMM_CHANNELS]


@pytest.mark.parametrize("geom,k,up,ci,co,settings", _IGEMM_CASES,
                         ids=[f"B{g[0]}T{g[1]}H{g[2]}W{g[3]}-k{'x'.join(map(str, k))}{'up' if up else ''}-{ci}to{co}"
                              for (g, k, up, ci, co, s) in _IGEMM_CASES])
def test_causal_igemm_kernels_bitwise(geom, k, up, ci, co, settings, monkeypatch):
    B, T, H, W = geom
    run, wants = _causal_case(B, T, H, W, ci, co, k, up, seed=100)
    taps = k[0] * k[1] * (k[2] if len(k) == 3 else 1)
    if taps * (R.pad64(ci) // 64) < 2:          # one K tile: the 8-phase form needs two and falls back to the setting's default
        settings = [(env, settings[0][1] if "LCV_CONV_8P" in env else name) for env, name in settings]
    _run_settings(run, wants, co, settings, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------
# row-tile kernel (csrc/conv_rows.h) and the implicit GEMM on the same data
# ---------------------------------------------------------------------------------------------------------------------------
def _rows_settings(co):
    rows = "conv_rows<256x16>" if co <= 16 else "conv_rows<256x96>"
    return [({}, rows), ({"LCV_CONV_ROWS_ORDER": "w"}, rows),
            ({"LCV_CONV_ROWS_GRID": "8"}, rows),               # one workgroup per XCD walks its tiles: next-tile prefetch, table parity
            ({"LCV_CONV_ROWS": "0"}, "conv16_igemm<128x128>")]


_ROWS_GEOMETRIES = [
    (2, 3, 4, 192),    # the smallest row the kernel accepts (75 % of one 256-pixel tile)
    (2, 3, 4, 256),    # exact tile
    (2, 3, 4, 384),    # second tile half empty; 48 tiles = six per XCD under LCV_CONV_ROWS_GRID=8
    (1, 1, 1, 200),    # one tile: seven of the eight XCDs get none
    (2, 1, 1, 192),    # two tiles, still fewer than the XCDs
]
_ROWS_CASES = [(g, k, False, ci, co) for g in _ROWS_GEOMETRIES
               for (k, ci, co) in (((3, 3, 3), 96, 96), ((3, 3, 3), 192, 96), ((3, 3, 3), 96, 3), ((3, 3, 3), 192, 48),
                                   ((1, 1, 1), 192, 96), ((1, 1, 1), 192, 48))]
# folded 2x upsample from W_in = 96 and 192: the output extents of the first and third geometry
_ROWS_CASES += [((2, 3, 2, win), (3, 3), True, ci, 96) for win in (96, 192) for ci in (192, 96)]


@pytest.mark.parametrize("geom,k,up,ci,co", _ROWS_CASES,
                         ids=[f"B{g[0]}T{g[1]}H{g[2]}W{g[3]}-k{'x'.join(map(str, k))}{'up' if up else ''}-{ci}to{co}"
                              for (g, k, up, ci, co) in _ROWS_CASES])
def test_row_tile_kernel_bitwise(geom, k, up, ci, co, monkeypatch):
    B, T, H, W = geom
    run, wants = _causal_case(B, T, H, W, ci, co, k, up, seed=200)
    _run_settings(run, wants, co, _rows_settings(co), monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------
# strided form (the encoder's downsampling stages)
# ---------------------------------------------------------------------------------------------------------------------------
_SAME_256 = [({}, "conv16_igemm<256x256>"), ({"LCV_CONV_N192": "2"}, "conv16_igemm<256x256>"),
             ({"LCV_CONV_N192": "3"}, "conv16_igemm<256x256>"), ({"LCV_CONV_N192": "0"}, "conv16_igemm<256x256>"),
             ({"LCV_CONV_8P": "1"}, "conv8p_igemm<256x256>")]
_STRIDED_CHANNELS = [(64, 64, _DEFAULT_128), (128, 192, _WIDE_192), (128, 256, _SAME_256)]
_STRIDED_GEOMETRIES = [
    # kernel, stride, (B, T, H, W) input, output extent
    ((3, 3), (1, 2, 2), (2, 3, 6, 10), (3, 3, 5)),
    ((3, 3), (1, 2, 2), (2, 3, 7, 9), (3, 3, 4)),
    ((3, 3), (1, 2, 2), (2, 3, 1, 1), (3, 1, 1)),
    ((3, 3), (1, 2, 2), (2, 3, 2, 3), (3, 1, 1)),
    ((3, 3), (1, 2, 2), (2, 3, 7, 9), (3, 2, 3)),          # an extent smaller than the largest legal one
    ((3, 1, 1), (2, 1, 1), (2, 3, 4, 5), (1, 4, 5)),       # Tout = (Tin - 1) / 2: the last tap of the last frame is the final input frame
    ((3, 1, 1), (2, 1, 1), (2, 5, 4, 5), (2, 4, 5)),
    ((3, 1, 1), (2, 1, 1), (2, 9, 4, 5), (4, 4, 5)),
    ((3, 1, 1), (2, 1, 1), (2, 9, 4, 5), (3, 4, 5)),       # one frame fewer
]
_STRIDED_CASES = [(k, s, g, o, ci, co, st) for (k, s, g, o) in _STRIDED_GEOMETRIES for (ci, co, st) in _STRIDED_CHANNELS]


@pytest.mark.parametrize("k,stride,geom,out_thw,ci,co,settings", _STRIDED_CASES,
                         ids=[f"k{'x'.join(map(str, k))}-in{'x'.join(map(str, g))}-out{'x'.join(map(str, o))}-{ci}to{co}"
                              for (k, s, g, o, ci, co, st) in _STRIDED_CASES])
def test_strided_kernels_bitwise(k, stride, geom, out_thw, ci, co, settings, monkeypatch):
    B, T, H, W = geom
    x, w, bias = R.make_x(B, ci, T, H, W, 300), R.make_w(co, ci, k, 301), R.make_bias(co, 302)
    R.check_data_rules(x, w, bias)
    want = R.to_kernel_layout(R.finish(R.strided_conv3d(x, w, stride, out_thw), bias))
    assert float(want.float().abs().max()) > 0
    conv, xc = _module(w, bias), R.to_kernel_layout(x).cuda()
    for env, name in settings:
        for kname, v in env.items():
            monkeypatch.setenv(kname, v)
        got = _vae()._conv_strided(xc, conv, stride, out_thw)
        assert _last_kernel() == name, (env, _last_kernel(), name)
        _assert_exact(got, want, co, env)
        for kname in env:
            monkeypatch.delenv(kname)


# ---------------------------------------------------------------------------------------------------------------------------
# batch independence of the whole VAE
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_vae():
    from longcat_video.modules.autoencoder_kl_wan import AutoencoderKLWan
    from oracle import vae_oracle as V
    cfg = V.default_config(base_dim=16, z_dim=4)
    vae = AutoencoderKLWan(base_dim=16, z_dim=4, device="cuda", dtype=BF16)
    state = dict(V.make_params(cfg, seed=3))
    state.update(V.make_encoder_params(cfg, seed=5))
    missing, unexpected = vae.load_state_dict(state, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return vae


def test_vae_decode_is_batch_independent():
    """decode of a batch of two equals the two single decodes bit for bit: no kernel in the path has a summation order that
    depends on where a pixel's tile lies, and every stage indexes the batch the way the single-sample call indexes sample 0."""
    vae = _oracle_vae()
    z = torch.randn(2, 4, 3, 6, 10, generator=torch.Generator().manual_seed(40)).to(BF16).cuda()
    both = vae.decode(z, return_dict=False)[0]
    assert both.shape == (2, 3, 9, 48, 80)
    singles = [vae.decode(z[b:b + 1].contiguous(), return_dict=False)[0] for b in range(2)]
    assert not torch.equal(singles[0], singles[1])
    for b in range(2):
        assert torch.equal(both[b:b + 1], singles[b]), f"sample {b}: {int((both[b:b + 1] != singles[b]).sum())} elements differ"


def test_vae_encode_is_batch_independent():
    vae = _oracle_vae()
    video = (torch.rand(2, 3, 9, 32, 48, generator=torch.Generator().manual_seed(41)) * 2 - 1).to(BF16).cuda()
    both = vae.encode(video).latent_dist.mode()
    assert both.shape == (2, 4, 3, 4, 6)
    singles = [vae.encode(video[b:b + 1].contiguous()).latent_dist.mode() for b in range(2)]
    assert not torch.equal(singles[0], singles[1])
    for b in range(2):
        assert torch.equal(both[b:b + 1], singles[b]), f"sample {b}: {int((both[b:b + 1] != singles[b]).sum())} elements differ"


# ---------------------------------------------------------------------------------------------------------------------------
# argument checks through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_einval_and_launch_nothing():
    from lcv_hip import lib as L
    lib = L.load()
    x = torch.zeros(2 * 3 * 5 * 7 * 64, dtype=BF16, device="cuda")
    w = torch.zeros(64 * 36 * 64, dtype=BF16, device="cuda")
    bias = torch.zeros(64, dtype=BF16, device="cuda")
    zero = torch.zeros(256, dtype=BF16, device="cuda")
    out = torch.full((2 * 3 * 5 * 7 * 64,), 7.0, dtype=BF16, device="cuda")
    ptr = lambda t: t.data_ptr()

    def causal(B=2, T=3, H=5, W=7, cin=64, cout=64, ldc=64, k=(3, 3, 3), up=0):
        return lib.lcv_causal_conv3d(ptr(x), ptr(w), ptr(bias), None, ptr(out), ptr(zero), B, T, H, W, cin, cout, ldc, k[0], k[1], k[2],
                                     up, None)

    def strided(B=2, T=3, H=5, W=7, cin=64, cout=64, ldc=64, k=(1, 3, 3), s=(1, 2, 2), o=(3, 2, 3)):
        return lib.lcv_conv3d_strided(ptr(x), ptr(w), ptr(bias), ptr(out), ptr(zero), B, T, H, W, cin, cout, ldc, k[0], k[1], k[2],
                                      s[0], s[1], s[2], o[0], o[1], o[2], None)

    bad = [
        ("36 taps", lambda: causal(k=(4, 3, 3)), "taps"),
        ("Cin % 32", lambda: causal(cin=48), "multiple of 32"),
        ("Cin % 32, strided", lambda: strided(cin=48), "multiple of 32"),
        ("even spatial kernel", lambda: causal(k=(3, 2, 3)), "odd spatial"),
        ("even spatial kernel", lambda: causal(k=(1, 3, 4)), "odd spatial"),
        ("ldc < Cout", lambda: causal(cout=64, ldc=32), "ldc"),
        ("ldc < Cout, strided", lambda: strided(cout=64, ldc=32), "ldc"),
        ("H extent past the input", lambda: strided(o=(3, 4, 3)), "past the input"),     # (4 - 1) * 2 = 6 >= 5
        ("W extent past the input", lambda: strided(o=(3, 2, 5)), "past the input"),     # (5 - 1) * 2 = 8 >= 7
        ("T extent past the input", lambda: strided(k=(3, 1, 1), s=(2, 1, 1), o=(3, 5, 7)), "past the input"),   # (3 - 1) * 2 = 4 >= 3
    ]
    for what, fn, needle in bad:
        assert fn() == -1, what                                          # LCV_EINVAL
        assert needle in lib.lcv_last_error().decode(), (what, lib.lcv_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                      # nothing ran
    assert causal(B=0) == 0 and strided(B=0) == 0                        # LCV_OK, and still nothing to write
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert causal() == 0 and strided() == 0                              # the same calls with legal arguments do run
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
