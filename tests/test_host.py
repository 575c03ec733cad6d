"""The shared host helpers (lightglue_amd/_host.py) and the pieces of the image-to-matches pipeline that need
no GPU: the argument check, the workspace carving's arithmetic, Features.rows and the package's names."""
import pytest
import torch


def test_require_gpu():
    from lightglue_amd import PluginError
    from lightglue_amd._host import require_gpu

    for bad in (torch.zeros(2, 3), [[1.0, 2.0]], None):
        with pytest.raises(PluginError, match="GPU") as e:
            require_gpu("logits", bad, "the keypoint front end", (torch.float16,), 2)
        assert all(s in str(e.value) for s in ("logits", "the keypoint front end", "no CPU fallback"))


def test_require_gpu_names_argument_and_dtypes():
    """The dtype and dim branch, reached without a GPU through a tensor subclass that claims to be on one."""
    from lightglue_amd._host import require_gpu

    class OnGpu(torch.Tensor):
        is_cuda = True

    t = torch.zeros(2, 3).as_subclass(OnGpu)
    require_gpu("x", t, "the stage")
    require_gpu("x", t, "the stage", (torch.float16, torch.float32), 2)
    with pytest.raises(ValueError, match="float16") as e:
        require_gpu("weight", t, "the stage", (torch.float16,))
    assert "weight" in str(e.value) and "torch.float16" in str(e.value) and "torch.float32" in str(e.value)
    with pytest.raises(ValueError, match="weight") as e:
        require_gpu("weight", t, "the stage", (torch.float16, torch.float32), 4)
    assert "torch.float16 or torch.float32" in str(e.value) and "4-d" in str(e.value) and "(2, 3)" in str(e.value)


def test_carve_offsets():
    from lightglue_amd._host import carve_offsets

    sizes = [1, 256, 257, 0, 4096]
    offsets, total = carve_offsets(sizes)
    assert offsets == [0, 256, 512, 1024, 1280] and total == 1280 + 4096
    assert all(o % 256 == 0 for o in offsets)
    assert all(a < b for a, b in zip(offsets, offsets[1:]))                       # strictly ordered
    assert all(o + n <= nxt for o, n, nxt in zip(offsets, sizes, offsets[1:] + [total]))  # no overlap
    assert total == sum((max(n, 1) + 255) // 256 * 256 for n in sizes)            # an empty region takes 256 too
    assert carve_offsets([]) == ([], 0)


def test_features_rows():
    from lightglue_amd import Features

    b, k = 4, 8
    gen = torch.Generator().manual_seed(11)
    f = Features(torch.randint(0, 99, (b, k, 2), generator=gen, dtype=torch.int32), torch.rand((b, k, 2), generator=gen),
                 torch.rand((b, k, 256), generator=gen), torch.rand((b, k), generator=gen),
                 torch.randint(0, k, (b,), generator=gen, dtype=torch.int32))
    for sl, want in ((slice(0, 2), Features(*(t[:2] for t in f))), (slice(2, 4), Features(*(t[2:] for t in f))),
                     (slice(2, None), Features(*(t[2:] for t in f)))):
        got = f.rows(sl)
        assert isinstance(got, Features)
        for name, x, y in zip(Features._fields, got, want):
            assert x.shape[0] == 2 and torch.equal(x, y), (sl, name)


def test_package_names():
    import lightglue_amd
    from lightglue_amd import _host, image, plugin

    assert plugin.PluginError is lightglue_amd.PluginError is _host.PluginError
    assert plugin._check is _host._check and plugin._workspace is _host._workspace
    assert not hasattr(image, "_Recording")
    assert "extract_pairs" in lightglue_amd.__all__ and callable(lightglue_amd.extract_pairs)
