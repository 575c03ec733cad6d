"""What tests/test_gpu_matcher_exact.py (the chained fp16 forward on the MI355X) and tests/test_matcher_reference.py
(the restatement, its bound and the mutants, no GPU) share: one TransformerLayer and the assignment head restated for
single pairs in plain tensor ops on the CPU, with the hip path's fp16 stores as a parameter. A plain module: no
fixtures, nothing here touches a GPU or reads anything but its arguments.

`rnd` is applied wherever the hip path rounds to fp16. rnd = ident gives *exact*: the reference's layer
(lightglue_pytorch_no_plugin/lightglue.py:88-233) on the fp16-rounded weights, unfolded, in the tensors' dtype
(float64). rnd = half gives the *storage model*: the same arithmetic with every fp16 store of the kernels. The same
function on float32 tensors with rnd = half is an fp32-arithmetic stand-in for the kernels (the CPU test's proxy).

The store points, each read from the kernel (csrc/):
  folded weights  weights._ffn_in_fused: [W_x | W_m W_p] and b + W_m b_p in fp32, then fp16 (_cached's .to(dtype));
                  the head's [W_final / 4 ; w_match] likewise (MatchAssignment.aug_weights)
  projections     fp16(acc + b), one rounding: lin_val, lightglue_device.h:84 (Wqkv, to_qk | to_v, the FFN's second
                  layer, the head's rows v; phase 3 of the FFN kernels: lightglue_ffn.hip:370 and :644-655)
  rotary          on that fp16 value, in fp16 arithmetic: both products and the sum rounded (rot_pair,
                  lightglue_device.h:126-133); v is the projection's fp16 value as it is
  attention       q~ = fp16(q * kScaleLog2), P = fp16(exp2(s - m)), the row sum and P V from that fp16 P, the context
                  fp16 (mha_hd64_device.h; tests/attention_refs.py states the kernels' arithmetic in full). The model
                  takes m as the row's true maximum; the kernels' m may trail it by up to 8 log2 units and the
                  single-pass kernels round P * alpha once more: roundings of the same size at other places
  FFN             h = fp16(acc + b1) BEFORE the LayerNorm, whose statistics come from that fp16 h
                  (lightglue_ffn.hip:33-36); fp16(GELU(LayerNorm(h))) (:263-264); y = fp16(acc + b2) (:300), then the
                  residual x' = fp16(y + x) as a second rounding (res_add, :313)
  the head        v = fp16(acc + b) for the 256 scaled channels and the matchability logit; the similarity is rounded
                  to fp16 as it leaves the MFMA accumulators ((f16)acc, lightglue_assign.hip:133: the reference's fp16
                  bmm), and both logsumexps and the combine 2 sim + row term + column term read that fp16 value; the
                  rest is fp32 arithmetic with no store

Mutants (`mutant=`): wiring errors between kernels that are each verified, for the CPU test to show that the bound
of the GPU test rejects them.
  fold_bias    out_proj's / to_out's bias lost in the FFN fold (b instead of b + W_m b_p; the stored forms only)
  rot_shift    the rotary tables read one row off            rot_v       the rotary applied to V as well
  self_all     self attention over both images' rows         cross_own   cross attention reads its own image's K, V
  no_residual  x' = ffn(...) without + x                      no_scale    scores without the 1/8
  cross_next   cross attention reads the NEXT pair's other image (needs P > 1)
  rot_other    cos / sin taken m rows further on (the other image's)
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

SCALE_LOG2 = float(np.float32(0.18033688011112042))   # kScaleLog2, the fp32 constant of mha_hd64_device.h
HEADS, HEAD_DIM, D = 4, 64, 256
LN_EPS = 1e-5
MUTANTS = ("fold_bias", "rot_shift", "rot_v", "self_all", "cross_own", "no_residual", "no_scale", "cross_next", "rot_other")

# The cases of both test files: name -> (pairs, m, n, per-pair descriptor scales or None). Pair p is
# synthetic_pair(300 + p, m, n, overlap = min(m, n) // 2).
CASES = {"a": (1, 40, 24, None), "b": (3, 150, 136, (1.0 / 16, 4.0, 1.0 / 16)), "c": (5, 150, 136, None),
         "d": (17, 128, 120, None), "e": (34, 128, 120, None)}
RAGGED_COUNTS = ([150, 120, 33], [136, 97, 120])   # on case b


def ident(t):
    return t


def half(t):
    """One fp16 store: round to nearest even, back in t's dtype."""
    return t.half().to(t.dtype)


def case_batch(name):
    """(kpts0 [P, m, 2], kpts1 [P, n, 2], desc0 [P, m, 256], desc1 [P, n, 256]) fp16 on the CPU."""
    from lightglue_amd import matcher

    pr, m, n, scales = CASES[name]
    pairs = [matcher.synthetic_pair(300 + p, m, n, overlap=min(m, n) // 2) for p in range(pr)]
    k0, k1, d0, d1 = (torch.cat(t, 0) for t in zip(*pairs))
    if scales is not None:
        s = torch.tensor(scales)[:, None, None]
        d0, d1 = d0 * s, d1 * s
    return tuple(t.half() for t in (k0, k1, d0, d1))


def pair_inputs(sd, k0, k1, d0, d1, dtype=torch.float64):
    """One pair's x [m + n, 256] and fp16 rotary tables cos, sin [m + n, 64] (FourierPositionalEncoding on the
    fp16-rounded Wr; the hip path stores both tables in fp16) from fp16 keypoints and descriptors [m, .], [n, .]."""
    wr = sd["posenc.Wr.weight"].half().double()
    proj = torch.cat((k0, k1), 0).double() @ wr.T
    cos = half(torch.cos(proj)).repeat_interleave(2, -1)
    sin = half(torch.sin(proj)).repeat_interleave(2, -1)
    return torch.cat((d0, d1), 0).to(dtype), cos.to(dtype), sin.to(dtype)


def _fold(w1, b1, wp, bp):
    """weights._ffn_in_fused: fp32 products, then the fp16 store."""
    w1, b1, wp, bp = (t.half().float() for t in (w1, b1, wp, bp))
    wx, wm = w1[:, :D], w1[:, D:]
    return torch.cat((wx, wm @ wp), 1).half(), (b1 + wm @ bp).half(), b1.half()


def layer_weights(sd, li, dtype=torch.float64):
    """Layer li's parameters from a state dict, fp16-rounded, in `dtype`, with the hip path's derived (folded) ones."""
    def g(name):
        return sd[f"transformers.{li}.{name}"].half()

    w = {}
    for blk, proj in (("self_attn", "out_proj"), ("cross_attn", "to_out")):
        b = {k: g(f"{blk}.{v}") for k, v in (("w1", "ffn.0.weight"), ("b1", "ffn.0.bias"), ("gamma", "ffn.1.weight"),
                                             ("beta", "ffn.1.bias"), ("w2", "ffn.3.weight"), ("b2", "ffn.3.bias"),
                                             ("wp", f"{proj}.weight"), ("bp", f"{proj}.bias"))}
        b["wf"], b["bf"], b["bf_nobias"] = _fold(b["w1"], b["b1"], b["wp"], b["bp"])
        w[blk] = {k: v.to(dtype) for k, v in b.items()}
    for k, v in (("wqkv", "self_attn.Wqkv.weight"), ("bqkv", "self_attn.Wqkv.bias"), ("wqk", "cross_attn.to_qk.weight"),
                 ("bqk", "cross_attn.to_qk.bias"), ("wv", "cross_attn.to_v.weight"), ("bv", "cross_attn.to_v.bias")):
        w[k] = g(v).to(dtype)
    return w


def head_weights(sd, li, dtype=torch.float64):
    """log_assignment[li]: the reference's parameters fp16-rounded, and MatchAssignment.aug_weights' [W / 4], b / 4
    (fp32 quotient, then fp16)."""
    g = {k: sd[f"log_assignment.{li}.{v}"].half() for k, v in (("wf", "final_proj.weight"), ("bf", "final_proj.bias"),
                                                                ("wm", "matchability.weight"), ("bm", "matchability.bias"))}
    g["wf4"], g["bf4"] = (g["wf"].float() / 4).half(), (g["bf"].float() / 4).half()
    return {k: v.to(dtype) for k, v in g.items()}


def rotary(t, cos, sin, rnd):
    """t [H, N, 64], cos / sin [N, 64]: t cos + swap(t) sin, swap((x0, x1)) = (-x1, x0), both products and the sum
    stored (rot_pair)."""
    pairs = t.unflatten(-1, (-1, 2))
    swapped = torch.stack((-pairs[..., 1], pairs[..., 0]), dim=-1).flatten(-2)
    return rnd(rnd(t * cos) + rnd(swapped * sin))


def attention(q, k, v, rnd, scale=True):
    """softmax(q k^T / 8) v for [H, nq, 64] x [H, nk, 64]. Stored form: the kernels' log2 domain with q~, P and the
    context rounded; exact form: the reference's."""
    if rnd is ident:
        s = (q / 8 if scale else q) @ k.transpose(-1, -2)
        p = torch.exp(s - s.max(-1, keepdim=True).values)
    else:
        s = rnd(q * (SCALE_LOG2 if scale else 8 * SCALE_LOG2)) @ k.transpose(-1, -2)
        p = rnd(torch.exp2(s - s.max(-1, keepdim=True).values))
    return rnd((p @ v) / p.sum(-1, keepdim=True))


def _merge(t):
    """[H, N, 64] -> [N, 256]."""
    return t.transpose(0, 1).reshape(t.shape[1], -1)


def _heads(t):
    """[N, 256] -> [H, N, 64]."""
    return t.view(t.shape[0], HEADS, HEAD_DIM).transpose(0, 1)


def ffn(b, x, msg, rnd, mutant=None):
    """x + ffn([x | proj(msg)]): the reference's block tail (exact), or the one-launch kernel's with the projection
    folded into the first weight and its four stores."""
    if rnd is ident:
        h = torch.cat((x, msg @ b["wp"].T + b["bp"]), -1) @ b["w1"].T + b["b1"]
        y = F.gelu(F.layer_norm(h, (2 * D,), b["gamma"], b["beta"], LN_EPS)) @ b["w2"].T + b["b2"]
        return y if mutant == "no_residual" else x + y
    bias = b["bf_nobias"] if mutant == "fold_bias" else b["bf"]
    h = rnd(torch.cat((x, msg), -1) @ b["wf"].T + bias)
    g = rnd(F.gelu(F.layer_norm(h, (2 * D,), b["gamma"], b["beta"], LN_EPS)))
    y = rnd(g @ b["w2"].T + b["b2"])
    return y if mutant == "no_residual" else rnd(y + x)


def layer(w, xs, tabs, dims, rnd=ident, mutant=None):
    """One TransformerLayer on a list of pairs: xs[p] [m_p + n_p, 256] (image 0's rows first), tabs[p] = (cos, sin)
    [m_p + n_p, 64], dims[p] = (m_p, n_p) -> the list of x'. The pairs meet only under mutant 'cross_next'."""
    scale = mutant != "no_scale"
    mid = []
    for x, (cos, sin), (m, n) in zip(xs, tabs, dims):
        t = rnd(x @ w["wqkv"].T + w["bqkv"]).view(m + n, HEADS, HEAD_DIM, 3).permute(3, 1, 0, 2)  # channel (h 64 + d) 3 + j
        if mutant == "rot_shift":
            cos, sin = torch.roll(cos, 1, 0), torch.roll(sin, 1, 0)
        if mutant == "rot_other":
            cos, sin = torch.roll(cos, -m, 0), torch.roll(sin, -m, 0)
        q, k = rotary(t[0], cos, sin, rnd), rotary(t[1], cos, sin, rnd)
        v = rotary(t[2], cos, sin, rnd) if mutant == "rot_v" else t[2]
        if mutant == "self_all":
            ctx = attention(q, k, v, rnd, scale)
        else:
            ctx = torch.cat([attention(q[:, :m], k[:, :m], v[:, :m], rnd, scale),
                             attention(q[:, m:], k[:, m:], v[:, m:], rnd, scale)], 1)
        x = ffn(w["self_attn"], x, _merge(ctx), rnd, mutant)
        mid.append((x, _heads(rnd(x @ w["wqk"].T + w["bqk"])), _heads(rnd(x @ w["wv"].T + w["bv"]))))
    out = []
    for p, ((x, qk, vv), (m, n)) in enumerate(zip(mid, dims)):
        if mutant == "cross_own":
            k0, v0, k1, v1 = qk[:, :m], vv[:, :m], qk[:, m:], vv[:, m:]
        else:
            o = (p + 1) % len(mid) if mutant == "cross_next" else p
            mo = dims[o][0]
            k0, v0, k1, v1 = mid[o][1][:, mo:], mid[o][2][:, mo:], mid[o][1][:, :mo], mid[o][2][:, :mo]
        msg = torch.cat([attention(qk[:, :m], k0, v0, rnd, scale), attention(qk[:, m:], k1, v1, rnd, scale)], 1)
        out.append(ffn(w["cross_attn"], x, _merge(msg), rnd, mutant))
    return out


def head(hw, x, m, rnd=ident):
    """MatchAssignment on one pair's x [m + n, 256] -> log-assignment scores [m, n] (lightglue.py:197-233). Stored
    form: the one projection with [W_final / 4 ; w_match] and its fp16 rows, and the fp16 similarity."""
    if rnd is ident:
        md = (x @ hw["wf"].T + hw["bf"]) / 4
    else:
        md = rnd(x @ hw["wf4"].T + hw["bf4"])
    z = rnd(x @ hw["wm"].T + hw["bm"])
    sim = rnd(md[:m] @ md[m:].T)
    return (F.log_softmax(sim, 1) + F.log_softmax(sim, 0) + F.logsigmoid(z[:m]) + F.logsigmoid(z[m:]).T)


def forward(layers, hw, xs, tabs, dims, rnd=ident, mutant=None, keep=None):
    """The whole forward on a list of pairs: every layer of `layers` (layer_weights), then the head `hw` ->
    (the final xs, the scores per pair). keep (a list): receives every layer's output list."""
    for w in layers:
        xs = layer(w, xs, tabs, dims, rnd, mutant)
        if keep is not None:
            keep.append(xs)
    return xs, [head(hw, x, m, rnd) for x, (m, _) in zip(xs, dims)]


def max_err(a, b):
    return float((a.double() - b.double()).abs().max())


def ffn_rows_form(rows):
    """Which one-launch FFN kernel launch_ffn_rows (lightglue_ffn.hip) takes for `rows` rows, with kTileGrid = 256
    (lightglue_device.h): 16-row tiles up to kRows16Round = 16 * 256 = 4096 rows, their projection split over two
    workgroups up to 64 tiles (ffn_split_parts); 32-row tiles up to kRows32Round = 32 * 256 = 8192 rows; 64-row
    tiles beyond."""
    if rows <= 16 * 256:
        return "rows16 split" if (rows + 15) // 16 <= 64 else "rows16"
    return "rows32" if rows <= 32 * 256 else "rows64"


assert math.isclose(SCALE_LOG2 * 8, math.log2(math.e), rel_tol=1e-7)
