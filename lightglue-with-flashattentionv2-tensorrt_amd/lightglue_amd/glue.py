"""ctypes wrappers of the gfx950 glue kernels around the attention op: one ``_Hip`` method per entry point."""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _lib
from ._host import DT, _workspace, call, stream_of
from .matches import MatchResult


def _sp(splits):
    """(n0, n1[, pairs]) -> (n0, n1, pairs): rows are `pairs` image pairs stacked pair-major."""
    return (splits[0], splits[1], splits[2] if len(splits) > 2 else 1)


def _mk(like: torch.Tensor, pr: int, heads: int, n: int) -> torch.Tensor:
    """One image's head-major tensor [P, heads, n, 64] in `like`'s dtype, on its device."""
    return torch.empty((pr, heads, n, 64), dtype=like.dtype, device=like.device)


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _Hip:
    """Thin wrappers of the gfx950 glue kernels (current stream, fail loudly on error). Row-major
    tensors hold P image pairs stacked pair-major ([1, P*(n0+n1), C]); per-image head-major
    tensors are [P, heads, ni, 64] (include/lightglue_glue.h)."""

    @staticmethod
    def qkv_rotary_split(qkv, cos, sin, heads, splits):
        n0, n1, pr = _sp(splits)
        out = [tuple(_mk(qkv, pr, heads, n) for _ in range(3)) for n in (n0, n1)]
        call("lg_qkv_rotary_split", DT[qkv.dtype], qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), heads, n0, n1, pr,
             *(t.data_ptr() for t in out[0]), *(t.data_ptr() for t in out[1]), stream_of(qkv))
        return out

    @staticmethod
    def split_heads2(a, b, heads, splits):
        n0, n1, pr = _sp(splits)
        a0, a1, b0, b1 = (_mk(a, pr, heads, n) for n in (n0, n1, n0, n1))
        call("lg_split_heads2", DT[a.dtype], a.data_ptr(), b.data_ptr(), heads, n0, n1, pr, a0.data_ptr(), a1.data_ptr(),
             b0.data_ptr(), b1.data_ptr(), stream_of(a))
        return (a0, a1), (b0, b1)

    @staticmethod
    def split_heads2_ld(ab, heads, splits):
        """ab [1, P*(N0+N1), 2*heads*64] = [a | b] (one GEMM's output) -> per image (a_i, b_i) heads."""
        n0, n1, pr = _sp(splits)
        a0, a1, b0, b1 = (_mk(ab, pr, heads, n) for n in (n0, n1, n0, n1))
        half = heads * 64
        call("lg_split_heads2_ld", DT[ab.dtype], ab.data_ptr(), ab.data_ptr() + half * ab.element_size(), 2 * half, heads,
             n0, n1, pr, a0.data_ptr(), a1.data_ptr(), b0.data_ptr(), b1.data_ptr(), stream_of(ab))
        return (a0, a1), (b0, b1)

    @staticmethod
    def merge_heads_cat(x, x0, x1):
        """[x | merge_heads(x0, x1)] -> [1, P*(N0+N1), 2*heads*64] (the FFN input)."""
        pr, heads, n0, n1 = x0.shape[0], x0.shape[1], x0.shape[2], x1.shape[2]
        out = torch.empty((1, pr * (n0 + n1), 2 * heads * 64), dtype=x.dtype, device=x.device)
        call("lg_merge_heads_cat", DT[x.dtype], x.data_ptr(), x0.data_ptr(), x1.data_ptr(), heads, n0, n1, pr,
             out.data_ptr(), stream_of(x))
        return out

    # ---- projections with their neighbours fused (fp16; csrc/lightglue_linear.hip, lightglue_ffn_ln.hip, lightglue_ffn.hip) ----
    @staticmethod
    def linear(a, w, b, res=None):
        """a [1, M, K] -> a·wᵀ + b (+ res) [1, M, N]."""
        m, k = a.shape[1], a.shape[2]
        out = torch.empty((1, m, w.shape[0]), dtype=a.dtype, device=a.device)
        call("lg_linear", a.data_ptr(), w.data_ptr(), b.data_ptr(), _ptr(res), m, w.shape[0], k, out.data_ptr(),
             stream_of(a))
        return out

    @staticmethod
    def linear_cat(x, c0, c1, w, b):
        """[x | merge_heads(c0, c1)]·wᵀ + b."""
        pr, heads, n0, n1 = c0.shape[0], c0.shape[1], c0.shape[2], c1.shape[2]
        out = torch.empty((1, pr * (n0 + n1), w.shape[0]), dtype=x.dtype, device=x.device)
        call("lg_linear_cat", x.data_ptr(), c0.data_ptr(), c1.data_ptr(), heads, n0, n1, pr, w.data_ptr(), b.data_ptr(),
             w.shape[0], out.data_ptr(), stream_of(x))
        return out

    @staticmethod
    def ffn(x, c0, c1, w, b, ln: nn.LayerNorm, w2, b2, packed=None):
        """x + ffn([x | merge_heads(c0, c1)]) (lightglue.py:101-106 with the block's residual):
        with `packed` (ffn_pack(w, w2)) one launch (ffn_rows_kernel), else linear_cat_ln_gelu into
        the scratch h, then linear(h, w2, b2, res=x) (include/lightglue_glue.h, lg_linear_set_ffn_fused)."""
        pr, heads, n0, n1 = c0.shape[0], c0.shape[1], c0.shape[2], c1.shape[2]
        m = pr * (n0 + n1)
        h = torch.empty((1, m, w.shape[0]), dtype=x.dtype, device=x.device)
        out = torch.empty((1, m, w2.shape[0]), dtype=x.dtype, device=x.device)
        call("lg_linear_cat_ffn", x.data_ptr(), c0.data_ptr(), c1.data_ptr(), heads, n0, n1, pr, w.data_ptr(), b.data_ptr(),
             ln.weight.data_ptr(), ln.bias.data_ptr(), float(ln.eps), w2.data_ptr(), b2.data_ptr(), _ptr(packed),
             h.data_ptr(), out.data_ptr(), stream_of(x))
        return out

    @staticmethod
    def ffn_proj(x, c0, c1, b, ln: nn.LayerNorm, b2, packed, kind, b3, splits, cos=None, sin=None, n_store=0):
        """lg_linear_cat_ffn_proj: (x' = x + ffn([x | merge_heads(c0, c1)]), the next projection of x')
        in one launch; kind 1 -> ((a0, a1), (b0, b1)) per-image heads (to_qk | to_v), kind 2 -> q/k/v
        per image with the rotary, kind 3 -> [1, M, n_store] rows."""
        n0, n1, pr = _sp(splits)
        heads = c0.shape[1]
        m = pr * (n0 + n1)
        out = torch.empty((1, m, 256), dtype=x.dtype, device=x.device)
        if kind == 1:
            outs = [_mk(x, pr, heads, n) for n in (n0, n1, n0, n1)]
        elif kind == 2:
            outs = [_mk(x, pr, heads, n) for n in (n0, n0, n0, n1, n1, n1)]
        else:
            outs = [torch.empty((1, m, n_store), dtype=x.dtype, device=x.device)]
        ptrs = (ctypes.c_void_p * 6)(*([t.data_ptr() for t in outs] + [None] * (6 - len(outs))))
        call("lg_linear_cat_ffn_proj", x.data_ptr(), c0.data_ptr(), c1.data_ptr(), heads, n0, n1, pr, b.data_ptr(),
             ln.weight.data_ptr(), ln.bias.data_ptr(), float(ln.eps), b2.data_ptr(), packed.data_ptr(), kind, b3.data_ptr(),
             _ptr(cos), _ptr(sin), n_store, ptrs, out.data_ptr(), stream_of(x))
        if kind == 1:
            return out, ((outs[0], outs[1]), (outs[2], outs[3]))
        if kind == 2:
            return out, [tuple(outs[:3]), tuple(outs[3:])]
        return out, outs[0]

    @staticmethod
    def linear_cat_ln_gelu(x, c0, c1, w, b, ln: nn.LayerNorm):
        """GELU(LayerNorm([x | merge_heads(c0, c1)]·wᵀ + b)) in one launch (P pairs of equal sizes)."""
        pr, heads, n0, n1 = c0.shape[0], c0.shape[1], c0.shape[2], c1.shape[2]
        out = torch.empty((1, pr * (n0 + n1), w.shape[0]), dtype=x.dtype, device=x.device)
        call("lg_linear_cat_ln_gelu", x.data_ptr(), c0.data_ptr(), c1.data_ptr(), heads, n0, n1, pr, w.data_ptr(),
             b.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(), float(ln.eps), out.data_ptr(), stream_of(x))
        return out

    @staticmethod
    def linear_qkv_rotary(x, w_perm, b_perm, cos, sin, heads, splits):
        n0, n1, pr = _sp(splits)
        out = [tuple(_mk(x, pr, heads, n) for _ in range(3)) for n in (n0, n1)]
        call("lg_linear_qkv_rotary", x.data_ptr(), w_perm.data_ptr(), b_perm.data_ptr(), cos.data_ptr(), sin.data_ptr(),
             heads, n0, n1, pr, x.shape[2], *(t.data_ptr() for t in out[0]), *(t.data_ptr() for t in out[1]),
             stream_of(x))
        return out

    @staticmethod
    def linear_split2(x, w, b, heads, splits):
        n0, n1, pr = _sp(splits)
        a0, a1, b0, b1 = (_mk(x, pr, heads, n) for n in (n0, n1, n0, n1))
        call("lg_linear_split2", x.data_ptr(), w.data_ptr(), b.data_ptr(), heads, n0, n1, pr, x.shape[2], a0.data_ptr(),
             a1.data_ptr(), b0.data_ptr(), b1.data_ptr(), stream_of(x))
        return (a0, a1), (b0, b1)

    @staticmethod
    def merge_heads(x0, x1):
        pr, heads, n0, n1 = x0.shape[0], x0.shape[1], x0.shape[2], x1.shape[2]
        out = torch.empty((1, pr * (n0 + n1), heads * 64), dtype=x0.dtype, device=x0.device)
        call("lg_merge_heads", DT[x0.dtype], x0.data_ptr(), x1.data_ptr(), heads, n0, n1, pr, out.data_ptr(),
             stream_of(x0))
        return out

    @staticmethod
    def layernorm_gelu(x, ln: nn.LayerNorm):
        y = torch.empty_like(x)
        rows, dim = x.numel() // x.shape[-1], x.shape[-1]
        call("lg_layernorm_gelu", DT[x.dtype], x.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(), rows, dim,
             float(ln.eps), y.data_ptr(), stream_of(x))
        return y

    @staticmethod
    def log_double_softmax(sim, z0, z1):
        """sim [P, m, n], z0 [P, m, 1], z1 [P, n, 1] (P pairs, one launch)."""
        pr, m, n = sim.shape[0], sim.shape[1], sim.shape[2]
        lib = _lib.load()
        out = torch.empty_like(sim)
        stream = stream_of(sim)
        ws = _workspace(sim.device, stream, lib.lg_log_double_softmax_workspace(m, n, pr))
        call("lg_log_double_softmax", sim.data_ptr(), z0.data_ptr(), z1.data_ptr(), m, n, pr, out.data_ptr(), ws.data_ptr(),
             stream)
        return out

    @staticmethod
    def log_double_softmax_f16(sim, v, m, zc):
        """sim [P, m, n] fp16 (contiguous); the matchability logits at channel zc of v [P, m + n, C]
        (the assignment projection's output): one fp32 scores tensor [P, m, n], two launches."""
        pr, n, ch = sim.shape[0], sim.shape[2], v.shape[2]
        lib = _lib.load()
        out = torch.empty(sim.shape, dtype=torch.float32, device=sim.device)
        stream = stream_of(sim)
        ws = _workspace(sim.device, stream, lib.lg_log_double_softmax_f16_workspace(m, n, pr))
        base = v.data_ptr() + zc * v.element_size()
        call("lg_log_double_softmax_f16", sim.data_ptr(), base, base + m * ch * v.element_size(), (m + n) * ch, ch, m, n, pr,
             out.data_ptr(), ws.data_ptr(), stream)
        return out

    _last_assign_ws = None  # (tests read the similarity copy the kernel leaves in its workspace)

    @staticmethod
    def assign_scores(v, m, zc, lens=None):
        """v [P, m + n, C] fp16: the assignment projection of both images' rows (scaled descriptors at
        channels 0..255, the matchability logit at zc) -> fp32 scores [P, m, n] (lg_assign_scores: the
        similarity and the dual log-softmax in two launches). lens = (m_len, n_len), int32 [P] on the
        device: the ragged form (lg_assign_scores_lens; -inf on padded rows and columns)."""
        pr, n, ch = v.shape[0], v.shape[1] - m, v.shape[2]
        lib = _lib.load()
        out = torch.empty((pr, m, n), dtype=torch.float32, device=v.device)
        stream = stream_of(v)
        ws = _workspace(v.device, stream, lib.lg_assign_scores_workspace(m, n, pr))
        _Hip._last_assign_ws = ws
        name, tables = ("lg_assign_scores", ()) if lens is None else ("lg_assign_scores_lens", [t.data_ptr() for t in lens])
        call(name, v.data_ptr(), (m + n) * ch, ch, zc, m, n, pr, *tables, out.data_ptr(), ws.data_ptr(), stream)
        return out

    @staticmethod
    def assign_matches(v, m, zc, threshold, lens=None):
        """v as for assign_scores -> MatchResult for all P pairs (lg_assign_matches: at most three
        launches, no fp32 scores tensor, no framework op, no host synchronisation). lens as for
        assign_scores (lg_assign_matches_lens: -1 / 0 on padded rows and columns)."""
        pr, n, ch = v.shape[0], v.shape[1] - m, v.shape[2]
        lib = _lib.load()
        out = MatchResult.empty(pr, m, n, v.device)
        stream = stream_of(v)
        ws = _workspace(v.device, stream, lib.lg_assign_matches_workspace(m, n, pr))
        name, tables = ("lg_assign_matches", ()) if lens is None else ("lg_assign_matches_lens", [t.data_ptr() for t in lens])
        call(name, v.data_ptr(), (m + n) * ch, ch, zc, m, n, pr, *tables, float(threshold), *(t.data_ptr() for t in out),
             ws.data_ptr(), stream)
        return out

    # ---- adaptive depth / width (csrc/lightglue_adaptive.hip) ----
    @staticmethod
    def token_scores(x, m, n, pr, lens, w_tok, b_tok, w_match, b_match, t_conf, t_keep, flags):
        """lg_token_scores on x [1, P*(m+n), 256]: (conf, mtch fp32 [P, m+n], keep uint8 [P, m+n], stats
        int32 [P, 4] = (kept0, kept1, unconfident, valid))."""
        dev = x.device
        conf = torch.empty((pr, m + n), dtype=torch.float32, device=dev)
        mtch = torch.empty_like(conf)
        keep = torch.empty((pr, m + n), dtype=torch.uint8, device=dev)
        stats = torch.empty((pr, 4), dtype=torch.int32, device=dev)
        lens = lens if lens is not None else (None, None)
        call("lg_token_scores", x.data_ptr(), m, n, pr, _ptr(lens[0]), _ptr(lens[1]), w_tok.data_ptr(), b_tok.data_ptr(),
             w_match.data_ptr(), b_match.data_ptr(), float(t_conf), float(t_keep), int(flags), conf.data_ptr(),
             mtch.data_ptr(), keep.data_ptr(), stats.data_ptr(), stream_of(x))
        return conf, mtch, keep, stats

    @staticmethod
    def compact_rows(x, cos, sin, keep, ind, m, n, pr, lens, m_out, n_out, prune=None, layers=0):
        """lg_compact_rows: the kept rows of x / cos / sin and of the index maps ind = (ind0, ind1) (None:
        identity) in the layout (m_out, n_out): (x, cos, sin, (ind0, ind1), (len0, len1)). prune = (prune0
        [P, m_orig], prune1 [P, n_orig]): the dropped rows' entries are set to `layers`."""
        dev = x.device
        rows = pr * (m_out + n_out)
        xo = torch.empty((1, rows, x.shape[2]), dtype=x.dtype, device=dev)
        co = torch.empty((1, rows, cos.shape[2]), dtype=cos.dtype, device=dev)
        so = torch.empty_like(co)
        i0, i1, l0, l1 = (torch.empty(s, dtype=torch.int32, device=dev) for s in ((pr, m_out), (pr, n_out), (pr,), (pr,)))
        lens = lens if lens is not None else (None, None)
        p0, p1 = prune if prune is not None else (None, None)
        call("lg_compact_rows", x.data_ptr(), cos.data_ptr(), sin.data_ptr(), keep.data_ptr(), _ptr(ind[0]), _ptr(ind[1]),
             m, n, pr, _ptr(lens[0]), _ptr(lens[1]), m_out, n_out, xo.data_ptr(), co.data_ptr(), so.data_ptr(),
             i0.data_ptr(), i1.data_ptr(), l0.data_ptr(), l1.data_ptr(), _ptr(p0), _ptr(p1),
             p0.shape[1] if p0 is not None else 0, p1.shape[1] if p1 is not None else 0, int(layers), stream_of(x))
        return xo, co, so, (i0, i1), (l0, l1)

    @staticmethod
    def matches_scatter(r, ind, lens, m, n, stop, prune=None):
        """lg_matches_scatter: the MatchResult r of the surviving rows (layout r.matches0.shape[1] x
        r.matches1.shape[1]) in the original layout m x n; prune's surviving entries are set to `stop`."""
        pr, mc, nc = r.matches0.shape[0], r.matches0.shape[1], r.matches1.shape[1]
        out = MatchResult.empty(pr, m, n, r.matches0.device)
        ind = ind if ind is not None else (None, None)
        lens = lens if lens is not None else (None, None)
        p0, p1 = prune if prune is not None else (None, None)
        call("lg_matches_scatter", *(t.data_ptr() for t in r), _ptr(ind[0]), _ptr(ind[1]), _ptr(lens[0]), _ptr(lens[1]),
             mc, nc, m, n, pr, int(stop), *(t.data_ptr() for t in out), _ptr(p0), _ptr(p1), stream_of(r.matches0))
        return out

    @staticmethod
    def pair_inputs(desc0, desc1, kpts0, kpts1, wr):
        """x [1, P*(m+n), 256] pair-major and the rotary tables cos, sin [1, P*(m+n), 64] in one launch."""
        pr, m, n, d = desc0.shape[0], desc0.shape[1], desc1.shape[1], desc0.shape[2]
        rows = pr * (m + n)
        x = torch.empty((1, rows, d), dtype=desc0.dtype, device=desc0.device)
        cos = torch.empty((1, rows, 64), dtype=desc0.dtype, device=desc0.device)
        sin = torch.empty_like(cos)
        t = [u.contiguous() for u in (desc0, desc1, kpts0, kpts1, wr)]
        call("lg_pair_inputs", *(u.data_ptr() for u in t), m, n, pr, d, x.data_ptr(), cos.data_ptr(), sin.data_ptr(),
             stream_of(desc0))
        return x, cos, sin
