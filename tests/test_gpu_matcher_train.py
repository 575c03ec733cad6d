"""LightGlueMatcher.loss: padding changes no bit of the loss or a gradient (TransformerLayer.forward_train's argument)."""
import numpy as np
import pytest
import torch

from gpu_common import same_bits, seeded_matcher
from lightglue_amd import matcher, synth

pytestmark = pytest.mark.gpu

P, M, OVERLAP = 2, 72, 30
COUNTS0, COUNTS1 = (72, 40), (64, 72)


def batch(pad):
    """fp16 (kpts0, kpts1, desc0, desc1) of P overlapping synthetic pairs, pad(shape) in the padded rows; gt0, gt1."""
    pairs = [matcher.synthetic_pair(11 + p, M, M, overlap=OVERLAP) for p in range(P)]
    ts = [torch.cat(t, 0) for t in zip(*pairs)]
    gt0, gt1 = (torch.full((P, M), -1, dtype=torch.int32) for _ in range(2))
    for p in range(P):  # synthetic_pair: column j < OVERLAP re-observes row src[j]
        src = torch.from_numpy(np.argsort(synth.uniform24((11 + p) * 4 + 5, M), kind="stable")[:OVERLAP].copy())
        gt0[p, src], gt1[p, :OVERLAP] = torch.arange(OVERLAP, dtype=torch.int32), src.int()
        for t, c in zip(ts, (COUNTS0[p], COUNTS1[p]) * 2):
            t[p, c:] = pad(t[p, c:].shape)
    return [t.half().cuda() for t in ts], gt0.cuda(), gt1.cuda()


def grads(model, pad, deep=True):
    inputs, gt0, gt1 = batch(pad)
    model.zero_grad(set_to_none=True)
    loss = model.loss(*inputs, gt0, gt1, counts0=list(COUNTS0), counts1=list(COUNTS1), deep=deep)
    loss.sum().backward()
    return loss.detach(), {name: p.grad for name, p in model.named_parameters()}


def test_padded_rows_change_no_bit_of_the_loss_or_the_gradients():
    model = seeded_matcher("cuda", n_layers=2).train()
    g = torch.Generator().manual_seed(3)
    loss, got = grads(model, torch.zeros)
    loss_r, got_r = grads(model, lambda shape: torch.randn(shape, generator=g))
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (P,) and same_bits(loss, loss_r)
    for name, grad in got.items():
        if name == "posenc.Wr.weight":
            assert grad is None
            continue
        assert grad is not None and bool(torch.isfinite(grad).all()) and bool((grad != 0).any()), name
        assert same_bits(grad, got_r[name]), name
    assert not torch.equal(loss, grads(model, torch.zeros, deep=False)[0])
