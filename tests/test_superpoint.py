"""The SuperPoint encoder's host side, no GPU: the framework restatement against a literal chain of ops, the
fp16-storage model, the weight packer and its inverse, every lg_sp_* entry point's argument check (nothing
reaches the device), and the state-dict and device checks of SuperPointEncoder."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

A = 4096  # a fake 16-B aligned address: never dereferenced on the paths below


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def sd():
    from lightglue_amd import seeded_superpoint_state_dict

    return seeded_superpoint_state_dict(3)


def image(seed, b, h, w):
    from lightglue_amd import synth

    return torch.from_numpy(synth.uniform24(seed, b * h * w).reshape(b, 1, h, w)).float()


def test_restatement_equals_the_literal_chain(sd):
    """superpoint_reference(storage=None) is superpoint.py:143-172 op for op: exact."""
    from lightglue_amd import superpoint_reference

    img = image(11, 2, 24, 40)

    def c(x, n):
        return F.conv2d(x, sd[f"{n}.weight"], sd[f"{n}.bias"], stride=1, padding=sd[f"{n}.weight"].shape[-1] // 2)

    x = F.relu(c(img, "conv1a"))
    x = F.relu(c(x, "conv1b"))
    x = F.max_pool2d(x, kernel_size=2, stride=2)
    x = F.relu(c(x, "conv2a"))
    x = F.relu(c(x, "conv2b"))
    x = F.max_pool2d(x, kernel_size=2, stride=2)
    x = F.relu(c(x, "conv3a"))
    x = F.relu(c(x, "conv3b"))
    x = F.max_pool2d(x, kernel_size=2, stride=2)
    x = F.relu(c(x, "conv4a"))
    x = F.relu(c(x, "conv4b"))
    scores = c(F.relu(c(x, "convPa")), "convPb")
    desc = c(F.relu(c(x, "convDa")), "convDb")
    logits, dense = superpoint_reference(sd, img)
    assert logits.shape == (2, 65, 3, 5) and dense.shape == (2, 256, 3, 5)
    assert torch.equal(logits, scores) and torch.equal(dense, desc)
    l3, d3 = superpoint_reference(sd, img[:, 0])  # [B, H, W] is taken as well
    assert torch.equal(l3, logits) and torch.equal(d3, dense)


def test_storage_model_rounds_and_stays_finite(sd):
    from lightglue_amd import superpoint_reference

    img = image(12, 1, 40, 72)
    sd16 = {k: v.half().double() for k, v in sd.items()}
    exact = superpoint_reference(sd16, img, None, torch.float64)
    model = superpoint_reference(sd, img, torch.float16, torch.float64)
    for e, m in zip(exact, model):
        assert m.dtype == torch.float64 and bool(torch.isfinite(m).all())
        assert torch.equal(m, m.half().double())  # every output is an fp16 value
        err = float((e - m).abs().max())
        assert 0.0 < err < 2e-2, err  # not a no-op, and a handful of fp16 roundings of values below 8
        assert float(e.abs().max()) < 6.0  # the seeded init neither saturates nor dies
        assert float(e.abs().max()) > 0.5


def test_seeded_state_dict_is_reproducible_and_he_normal(sd):
    from lightglue_amd import seeded_superpoint_state_dict
    from lightglue_amd.superpoint import LAYERS

    again = seeded_superpoint_state_dict(3)
    other = seeded_superpoint_state_dict(4)
    assert sorted(sd) == sorted(f"{n}.{k}" for n in LAYERS for k in ("weight", "bias"))
    for k in sd:
        assert torch.equal(sd[k], again[k]) and not torch.equal(sd[k], other[k])
    w = sd["conv3b.weight"]
    assert w.shape == (128, 128, 3, 3) and abs(float(w.std()) / np.sqrt(2.0 / (128 * 9)) - 1.0) < 0.02
    assert abs(float(sd["convDb.bias"].std()) / 0.1 - 1.0) < 0.2


@pytest.mark.parametrize("cin,cout,k", [(ci, co, 3) for ci in (64, 128) for co in (64, 128, 256, 512)] + [(256, 352, 1)])
def test_packer_roundtrip_and_fragment_order(lib, cin, cout, k):
    from lightglue_amd.superpoint import pack_conv, unpack_conv

    w = torch.arange(cout * cin * k * k, dtype=torch.float32).reshape(cout, cin, k, k)
    p = pack_conv(w)
    assert p.dim() == 1 and p.numel() * 2 == lib.lg_sp_packed_bytes(k * k, cin, cout)
    assert torch.equal(unpack_conv(p, cout, cin, k, k), w)
    # the header's formula: element (cb, t, ks, hi, r, j) = weight[32 cb + r][16 ks + 8 hi + j][t / k][t % k]
    v = p.reshape(cout // 32, k * k, cin // 16, 2, 32, 8)
    rng = np.random.default_rng(cin + cout)
    for _ in range(50):
        cb, t, ks = int(rng.integers(cout // 32)), int(rng.integers(k * k)), int(rng.integers(cin // 16))
        hi, r, j = int(rng.integers(2)), int(rng.integers(32)), int(rng.integers(8))
        assert v[cb, t, ks, hi, r, j] == w[32 * cb + r, 16 * ks + 8 * hi + j, t // k, t % k]


def test_packed_bytes_rejects_unsupported_layers(lib):
    assert lib.lg_sp_packed_bytes(9, 64, 64) == 9 * 64 * 64 * 2 and lib.lg_sp_packed_bytes(9, 128, 512) == 9 * 128 * 512 * 2
    assert lib.lg_sp_packed_bytes(1, 256, 352) == 256 * 352 * 2
    for bad in ((9, 32, 64), (9, 64, 96), (9, 256, 256), (9, 64, 1024), (1, 256, 256), (1, 128, 352), (4, 64, 64), (0, 64, 64),
                (9, -64, 64), (9, 64, 0)):
        assert lib.lg_sp_packed_bytes(*bad) == 0, bad


def _rejects(call, bads):
    for bad in bads:
        assert call(**bad) == 1, bad


def test_entry_points_validate_before_touching_the_device(lib):
    """lg_sp_conv1, lg_sp_conv3x3, lg_sp_heads: an empty launch returns success and every clause of the
    argument check rejects with a message, on fake addresses and without a device call."""
    from lightglue_amd import _lib

    def conv1(**kw):
        a = dict(dt=1, img=A, w=A, b=A, h=8, wd=8, batch=0, flags=1, out=2 * A)
        a.update(kw)
        return lib.lg_sp_conv1(a["dt"], a["img"], a["w"], a["b"], a["h"], a["wd"], a["batch"], a["flags"], a["out"], None)

    assert conv1() == 0 and conv1(dt=0, flags=0, img=A + 4, w=A + 16, b=A + 16, h=1, wd=3) == 0
    _rejects(conv1, [dict(dt=2), dict(dt=-1), dict(img=None), dict(w=None), dict(b=None), dict(out=None), dict(img=A + 1),
                     dict(dt=0, img=A + 2), dict(w=A + 8), dict(b=A + 8), dict(out=2 * A + 8), dict(out=A), dict(h=0),
                     dict(wd=0), dict(h=-8), dict(wd=-8), dict(batch=-1), dict(batch=65536), dict(flags=2), dict(flags=4),
                     dict(h=1 << 14, wd=1 << 13), dict(batch=2, h=1 << 15, wd=1 << 15)])
    assert "lg_sp_conv1" in _lib.last_error()

    def conv(**kw):
        a = dict(x=A, w=A, b=A, cin=64, cout=64, h=8, wd=8, batch=0, flags=3, out=2 * A)
        a.update(kw)
        return lib.lg_sp_conv3x3(a["x"], a["w"], a["b"], a["cin"], a["cout"], a["h"], a["wd"], a["batch"], a["flags"], a["out"],
                                 None)

    assert conv() == 0 and conv(cin=128, cout=512, flags=0, h=3, wd=5, b=A + 8) == 0 and conv(flags=1, h=1, wd=1) == 0
    for cin in (64, 128):
        for cout in (64, 128, 256, 512):
            assert conv(cin=cin, cout=cout) == 0
    _rejects(conv, [dict(cin=32), dict(cin=96), dict(cin=256), dict(cin=0), dict(cin=-64), dict(cout=32), dict(cout=65),
                    dict(cout=192), dict(cout=1024), dict(cout=0), dict(h=3), dict(wd=5), dict(flags=2, h=8, wd=7),
                    dict(flags=4), dict(flags=-1), dict(x=None), dict(w=None), dict(b=None), dict(out=None), dict(x=A + 8),
                    dict(w=A + 8), dict(b=A + 4), dict(out=2 * A + 8), dict(out=A), dict(h=0), dict(wd=0), dict(h=-2),
                    dict(wd=-2), dict(batch=-1), dict(batch=65536), dict(h=1 << 14, wd=1 << 13),
                    dict(batch=2, h=1 << 15, wd=1 << 15)])
    assert "lg_sp_conv3x3" in _lib.last_error()

    def heads(**kw):
        a = dict(x=A, w=A, b=A, hc=4, wc=4, batch=0, logits=2 * A, dense=3 * A)
        a.update(kw)
        return lib.lg_sp_heads(a["x"], a["w"], a["b"], a["hc"], a["wc"], a["batch"], a["logits"], a["dense"], None)

    assert heads() == 0 and heads(hc=1, wc=1, logits=2 * A + 2, dense=3 * A + 8, b=A + 8) == 0
    _rejects(heads, [dict(x=None), dict(w=None), dict(b=None), dict(logits=None), dict(dense=None), dict(x=A + 8), dict(w=A + 8),
                     dict(b=A + 4), dict(logits=2 * A + 1), dict(dense=3 * A + 4), dict(dense=A), dict(logits=A),
                     dict(logits=3 * A), dict(hc=0), dict(wc=0), dict(hc=-1), dict(wc=-4), dict(batch=-1), dict(batch=65536),
                     dict(hc=1 << 11, wc=1 << 10), dict(batch=2, hc=1 << 12, wc=1 << 12)])
    assert "lg_sp_heads" in _lib.last_error()


def test_state_dict_and_device_checks(sd):
    from lightglue_amd import PluginError, SuperPointEncoder, superpoint_reference

    enc = SuperPointEncoder(sd)  # (packs nothing yet: the weights go to a device at the first call there)
    missing = {k: v for k, v in sd.items() if k != "conv3a.bias"}
    with pytest.raises(KeyError, match="conv3a.bias"):
        SuperPointEncoder(missing)
    with pytest.raises(KeyError, match="conv3a.bias"):
        superpoint_reference(missing, image(1, 1, 8, 8))
    for key, shape in (("convPb.weight", (64, 256, 1, 1)), ("conv1a.weight", (64, 3, 3, 3)), ("conv4b.bias", (64,)),
                       ("convDa.weight", (256, 128, 1, 1))):
        bad = dict(sd)
        bad[key] = torch.zeros(shape)
        with pytest.raises(ValueError, match=key):
            SuperPointEncoder(bad)
    bad = dict(sd)
    bad["conv2a.weight"] = [1.0]
    with pytest.raises(ValueError, match="conv2a.weight"):
        SuperPointEncoder(bad)
    with pytest.raises(ValueError, match="float16"):
        SuperPointEncoder(sd, dtype=torch.float32)
    with pytest.raises(PluginError, match="GPU"):
        enc.heads(image(1, 1, 8, 8))
    with pytest.raises(PluginError, match="GPU"):
        enc.heads(image(1, 1, 8, 8).half()[:, 0])


def test_cpu_tensors_fail_loudly_in_every_stage(sd):
    from lightglue_amd import PluginError, superpoint

    x = torch.zeros(1, 8, 8, 64, dtype=torch.float16)
    w = torch.zeros(9 * 64 * 64, dtype=torch.float16)
    b = torch.zeros(64, dtype=torch.float16)
    with pytest.raises(PluginError, match="GPU"):
        superpoint.conv1(torch.zeros(1, 8, 8), torch.zeros(64, 1, 3, 3, dtype=torch.float16), b)
    with pytest.raises(PluginError, match="GPU"):
        superpoint.conv3x3(x, w, b)
    with pytest.raises(PluginError, match="GPU"):
        superpoint.heads(torch.zeros(1, 1, 1, 512, dtype=torch.float16), torch.zeros(352 * 256, dtype=torch.float16),
                         torch.zeros(352, dtype=torch.float16))
