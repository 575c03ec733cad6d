"""A/B of lg_assign_nll (loss and dloss/dv in one call) against the same loss and its backward in fp16 framework
ops on the GPU, both timed as graph replays; then the gradient kernel's split candidates (LG_ASSIGN_NLL_SPLITS)
and the loss-only call (statistics + terms) at 1 x 1024^2. One JSON line per measurement:

    python tools/assign_nll_ab.py > profiles/assign_nll/ab.jsonl
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd"))

from lightglue_amd.glue import _Hip  # noqa: E402

LD, ZC = 384, 256
SHAPES = ((1, 1024, 1024), (1, 2048, 2048), (16, 1024, 1024))


def operands(pr, m, n):
    """v fp16 [P, m + n, LD] (unit-norm descriptors times 4, normal logits); half the rows positive on distinct
    columns, a quarter unmatchable, the rest ignored; the unclaimed columns unmatchable."""
    g = torch.Generator().manual_seed(pr * 7 + m)
    v = torch.zeros((pr, m + n, LD))
    v[:, :, :256] = F.normalize(torch.randn((pr, m + n, 256), generator=g), dim=-1) * 4.0
    v[:, :, ZC] = torch.randn((pr, m + n), generator=g)
    gt0, gt1 = torch.full((pr, m), -2, dtype=torch.int32), torch.full((pr, n), -1, dtype=torch.int32)
    for p in range(pr):
        rows, cols = torch.randperm(m, generator=g), torch.randperm(n, generator=g)
        gt0[p, rows[:m // 2]] = cols[:m // 2].int()
        gt0[p, rows[m // 2:m // 2 + m // 4]] = -1
        gt1[p, cols[:m // 2]] = -2
    return v.half().cuda(), gt0.cuda(), gt1.cuda()


def framework(v, m, gt0, gt1):
    """The loss in fp16 framework ops (the scores as the fp16 model forms them) and its autograd backward -> dv."""
    leaf = v.detach().requires_grad_()
    m0, m1 = leaf[:, :m, :256], leaf[:, m:, :256]
    sim = m0 @ m1.transpose(1, 2)
    s = (F.log_softmax(sim, 2) + F.log_softmax(sim, 1) + F.logsigmoid(leaf[:, :m, ZC])[:, :, None] +
         F.logsigmoid(leaf[:, m:, ZC])[:, None, :])
    pos = gt0 >= 0
    picked = s.gather(2, gt0.clamp_min(0).long()[:, :, None])[:, :, 0]
    n0, n1 = gt0 == -1, gt1 == -1
    neg = (F.logsigmoid(-leaf[:, :m, ZC]) * n0).sum(1) + (F.logsigmoid(-leaf[:, m:, ZC]) * n1).sum(1)
    loss = (-0.5 * (picked * pos).sum(1) / pos.sum(1).clamp_min(1) - 0.5 * neg / (n0.sum(1) + n1.sum(1)).clamp_min(1))
    loss.float().sum().backward()
    return loss, leaf.grad


def graph_us(run, replays=50, rounds=5):
    """Median over rounds of the mean replay time of run() captured in a graph (microseconds)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run()
    times = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        graph.replay()
        t0.record()
        for _ in range(replays):
            graph.replay()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1000.0 / replays)
    return sorted(times)[len(times) // 2], times


def emit(**row):
    print(json.dumps(row), flush=True)


def main():
    for pr, m, n in SHAPES:
        v, gt0, gt1 = operands(pr, m, n)
        with torch.no_grad():
            new, new_all = graph_us(lambda: _Hip.assign_nll(v, m, ZC, gt0, gt1))
        old, old_all = graph_us(lambda: framework(v, m, gt0, gt1))
        emit(what="ab", shape=[pr, m, n], hip_us=round(new, 2), framework_us=round(old, 2), ratio=round(old / new, 3),
             hip_rounds=[round(t, 2) for t in new_all], framework_rounds=[round(t, 2) for t in old_all])
    pr, m, n = SHAPES[0]
    v, gt0, gt1 = operands(pr, m, n)
    with torch.no_grad():
        for g in (1, 2, 4, 8):
            os.environ["LG_ASSIGN_NLL_SPLITS"] = str(g)
            us, _ = graph_us(lambda: _Hip.assign_nll(v, m, ZC, gt0, gt1))
            emit(what="splits", shape=[pr, m, n], splits=g, hip_us=round(us, 2))
        del os.environ["LG_ASSIGN_NLL_SPLITS"]
        us, _ = graph_us(lambda: _Hip.assign_nll(v, m, ZC, gt0, gt1, need_grad=False))
        emit(what="loss_only", shape=[pr, m, n], hip_us=round(us, 2))
        us, _ = graph_us(lambda: _Hip.assign_scores(v, m, ZC))
        emit(what="assign_scores", shape=[pr, m, n], hip_us=round(us, 2))


if __name__ == "__main__":
    main()
