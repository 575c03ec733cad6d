"""A/B of lg_proj_backward (full and data gradient only) per kind against the same gradients in fp16 framework ops
(un-rotate, merge heads, two matmuls and a column sum), all graph replays, alternated round by round in one process, at
2,048 rows (one pair of 1,024 keypoints) and 32,768 rows (16 pairs); then the weight kernel's split candidates
(LG_PROJ_BACKWARD_SPLITS) at both sizes and at 320 and 640 rows, the small end of the rule. One JSON line per
measurement:

    python tools/proj_backward_ab.py > profiles/proj_backward/ab.jsonl
"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd"))

from lightglue_amd.glue import _Hip  # noqa: E402

SHAPES = ((1, 1024, 1024), (16, 1024, 1024))
KINDS = {"split2": (1, 512), "qkv": (2, 768), "plain": (3, 384)}


def operands(kind, pr, n0, n1):
    g = torch.Generator().manual_seed(pr)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    m, n = pr * (n0 + n1), KINDS[kind][1]
    t = dict(x=rn(1, m, 256).half(), w=(rn(n, 256) / 16).half())
    if kind == "plain":
        t["grads"] = [rn(m, 384) / 16]
    else:
        t["grads"] = [(rn(pr, 4, ni, 64) / 16).half() for ni in ((n0, n0, n0, n1, n1, n1) if kind == "qkv" else (n0, n1, n0, n1))]
    if kind == "qkv":
        ang = 6.0 * rn(1, m, 32)
        t["cos"], t["sin"] = (f(ang).repeat_interleave(2, -1).half() for f in (torch.cos, torch.sin))
    return {k: [g.cuda() for g in v] if k == "grads" else v.cuda() for k, v in t.items()}


def framework(kind, t, full):
    """dx (and dw, db) in fp16 framework ops: the merge as one permute per image tensor and a cat, the transposed
    rotary as layers._rotary writes the forward's."""
    g = t["grads"]
    merge = lambda a, b: torch.cat((a.permute(0, 2, 1, 3).flatten(2), b.permute(0, 2, 1, 3).flatten(2)), 1).flatten(0, 1)  # noqa: E731
    if kind == "plain":
        G = g[0].half()
    elif kind == "split2":
        G = torch.cat((merge(g[0], g[1]), merge(g[2], g[3])), 1)
    else:
        c, s = t["cos"][0].repeat(1, 4), t["sin"][0].repeat(1, 4)
        parts = []
        for j in range(2):
            v = merge(g[j], g[3 + j])
            p = v.unflatten(-1, (-1, 2))
            parts.append(v * c + torch.stack((p[..., 1], -p[..., 0]), -1).flatten(-2) * s)
        G = torch.cat(parts + [merge(g[2], g[5])], 1)
    dx = G @ t["w"]
    return (dx, G.T @ t["x"][0], G.sum(0)) if full else (dx,)


def capture(run):
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
    return graph


def replay_us(graph, replays):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    graph.replay()
    t0.record()
    for _ in range(replays):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0 / replays


def emit(**row):
    print(json.dumps(row), flush=True)


def hip(kind, t, splits, need):
    return _Hip.proj_backward(KINDS[kind][0], t["x"], t["w"], t["grads"], splits, t.get("cos"), t.get("sin"), KINDS[kind][1],
                              None, need)


@torch.no_grad()
def main():
    for pr, n0, n1 in SHAPES:
        for kind in KINDS:
            t, sp = operands(kind, pr, n0, n1), (n0, n1, pr)
            graphs = {"hip_full": capture(lambda: hip(kind, t, sp, True)), "hip_data": capture(lambda: hip(kind, t, sp, False)),
                      "fw_full": capture(lambda: framework(kind, t, True)), "fw_data": capture(lambda: framework(kind, t, False))}
            replays = 50 if pr == 1 else 10
            rounds = {k: [] for k in graphs}
            for _ in range(5):
                for k, g in graphs.items():
                    rounds[k].append(replay_us(g, replays))
            emit(what="ab", kind=kind, rows=pr * (n0 + n1), **{k + "_us": round(sorted(v)[2], 2) for k, v in rounds.items()},
                 spread_us={k: round(max(v) - min(v), 2) for k, v in rounds.items()},
                 rounds_us={k: [round(x, 2) for x in v] for k, v in rounds.items()})
            for s in (1, 4, 8, 16, 20, 32, 40, 64):
                os.environ["LG_PROJ_BACKWARD_SPLITS"] = str(s)
                g = capture(lambda: hip(kind, t, sp, True))
                emit(what="splits", kind=kind, rows=pr * (n0 + n1), splits=s,
                     hip_full_us=round(sorted(replay_us(g, replays) for _ in range(3))[1], 2))
            del os.environ["LG_PROJ_BACKWARD_SPLITS"]
    for n0, n1 in ((150, 170), (320, 320)):   # the small end of the rule
        for kind in KINDS:
            t = operands(kind, 1, n0, n1)
            for s in (1, 2, 4, 10, 20, 40):
                os.environ["LG_PROJ_BACKWARD_SPLITS"] = str(s)
                g = capture(lambda: hip(kind, t, (n0, n1, 1), True))
                emit(what="threshold", kind=kind, rows=n0 + n1, splits=s,
                     hip_full_us=round(sorted(replay_us(g, 50) for _ in range(3))[1], 2))
            del os.environ["LG_PROJ_BACKWARD_SPLITS"]


if __name__ == "__main__":
    main()
