"""A/B of lg_ffn_backward (full and data gradients only) against the backward of the same block in fp16 framework ops
(forward + backward minus forward), all graph replays, alternated round by round in one process, at 2,048 rows (one
pair of 1,024 keypoints) and 32,768 rows (16 pairs); then the weight kernel's split candidates
(LG_FFN_BACKWARD_SPLITS) at both sizes and at 320 and 640 rows, either side of the rule's threshold. One JSON line per
measurement:

    python tools/ffn_backward_ab.py > profiles/ffn_backward/ab.jsonl
"""
import json
import math
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd"))

from lightglue_amd.glue import _Hip  # noqa: E402

SHAPES = ((1, 1024, 1024), (16, 1024, 1024))
EPS = 1e-5


def operands(pr, n0, n1):
    g = torch.Generator().manual_seed(pr)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = dict(x=rn(1, pr * (n0 + n1), 256), ctx0=rn(pr, 4, n0, 64), ctx1=rn(pr, 4, n1, 64), w1=rn(512, 512) / math.sqrt(512),
             b1=0.1 * rn(512), gamma=1 + 0.1 * rn(512), beta=0.1 * rn(512), w2=rn(256, 512) / math.sqrt(512), b2=0.1 * rn(256),
             dy=rn(1, pr * (n0 + n1), 256) / 16)
    return {k: v.half().cuda() for k, v in t.items()}


def framework(t, backward):
    """The block in fp16 framework ops on leaves (the merge included, as the kernels gather it) and, with backward,
    its autograd."""
    d = {k: v.detach().requires_grad_(backward) for k, v in t.items() if k != "dy"}
    heads = [v.permute(0, 2, 1, 3).flatten(2) for v in (d["ctx0"], d["ctx1"])]   # one permute per image tensor
    merged = torch.cat(heads, 1).flatten(0, 1)
    c = torch.cat((d["x"][0], merged), 1)
    h = F.gelu(F.layer_norm(F.linear(c, d["w1"], d["b1"]), (512,), d["gamma"], d["beta"], EPS))
    out = d["x"][0] + F.linear(h, d["w2"], d["b2"])
    if backward:
        out.backward(t["dy"][0])
    return out


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


def main():
    for pr, n0, n1 in SHAPES:
        t = operands(pr, n0, n1)
        ln = SimpleNamespace(weight=t["gamma"], bias=t["beta"], eps=EPS)
        hip = lambda need: _Hip.ffn_backward(t["x"], t["ctx0"], t["ctx1"], t["w1"], t["b1"], ln, t["w2"], t["dy"], need)  # noqa: E731
        with torch.no_grad():
            graphs = {"hip_full": capture(lambda: hip(True)), "hip_data": capture(lambda: hip(False)),
                      "fw_forward": capture(lambda: framework(t, False))}
        graphs["fw_both"] = capture(lambda: framework(t, True))
        replays = 50 if pr == 1 else 10
        rounds = {k: [] for k in graphs}
        for _ in range(5):
            for k, g in graphs.items():
                rounds[k].append(replay_us(g, replays))
        med = {k: sorted(v)[2] for k, v in rounds.items()}
        spread = {k: max(v) - min(v) for k, v in rounds.items()}
        emit(what="ab", rows=pr * (n0 + n1), hip_full_us=round(med["hip_full"], 2), hip_data_us=round(med["hip_data"], 2),
             framework_backward_us=round(med["fw_both"] - med["fw_forward"], 2),
             spread_us={k: round(v, 2) for k, v in spread.items()}, rounds_us={k: [round(x, 2) for x in v] for k, v in rounds.items()})
        with torch.no_grad():
            for s in (1, 4, 8, 10, 16, 20):
                os.environ["LG_FFN_BACKWARD_SPLITS"] = str(s)
                g = capture(lambda: hip(True))
                emit(what="splits", rows=pr * (n0 + n1), splits=s, hip_full_us=round(sorted(replay_us(g, replays) for _ in range(3))[1], 2))
            del os.environ["LG_FFN_BACKWARD_SPLITS"]
    for n0, n1 in ((150, 170), (320, 320)):   # either side of the rule's 320-row threshold
        t = operands(1, n0, n1)
        ln = SimpleNamespace(weight=t["gamma"], bias=t["beta"], eps=EPS)
        with torch.no_grad():
            for s in (1, 2, 4, 10, 20):
                os.environ["LG_FFN_BACKWARD_SPLITS"] = str(s)
                g = capture(lambda: _Hip.ffn_backward(t["x"], t["ctx0"], t["ctx1"], t["w1"], t["b1"], ln, t["w2"], t["dy"], True))
                emit(what="threshold", rows=n0 + n1, splits=s, hip_full_us=round(sorted(replay_us(g, 50) for _ in range(3))[1], 2))
            del os.environ["LG_FFN_BACKWARD_SPLITS"]


if __name__ == "__main__":
    main()
