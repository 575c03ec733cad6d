"""The assignment head, the match head, the two dual log-softmax entry points and lg_pair_inputs on the MI355X
(csrc/lightglue_assign.hip, csrc/lightglue_glue.hip) against float64 references computed on the CPU from the operands
the kernels read (tests/assignment_refs.py: the operation, the input sets and the derivation of the per-element bound).
tests/test_assignment_reference.py shows without a GPU that the bound accepts each kernel's arithmetic restated in fp32
and rejects the plausible wrong kernels, that the shapes below reach the paths named, and that no row of the match
head's inputs lies near a tie or a threshold. Nothing here reads a similarity or a score back from a kernel to build an
expectation.

Calls go through lightglue_amd._host.call on raw pointers. Every output (the scores, each of the match head's seven)
and the workspace is a view inside a larger allocation filled with a sentinel byte, 4 KiB of it on both sides: after
the call the guards are unchanged (the workspace's tail past lg_*_workspace() bytes included) and no output element
still holds the sentinel. v has NaN before and behind it (gpu_common.GuardedIn), and the padded rows of a ragged pair
hold NaN and +-Inf.

Shapes (P, m, n), from assign_splits / launch_assign_lse / assign_scores_run, dual_ws_stride's chunks and ds_small:

  lg_assign_scores[_lens]   (1, 1, 8) S = 8 with every share but the first empty; (1, 33, 72) S = 8 and a row tail;
                            (3, 300, 296) S = 4, BPW 1; (1, 8, 1032) S = 4, BPW 2; (1, 40, 2048) S = 2, BPW 4;
                            (3, 8, 2048) S = 1, BPW 8, the 8-row combine; (2, 2048, 8) S = 1, the 32-row combine;
                            (1, 70, 520) a second 512-column block. Each also ragged (assignment_refs.ragged_counts:
                            counts that cut a 32-row strip and a lane's 8 columns and leave whole blocks in padding).
  lg_log_double_softmax     (1, 1, 1); (1, 3, 5) fewer rows than the 4-row interleave; (1, 129, 65) a second chunk of
                            one row and a ragged 64-column group; (3, 130, 257).
  lg_log_double_softmax_f16 small form: (1, 9, 8), (1, 9, 520), (1, 9, 1032) CPL 1 / 2 / 4; (1, 1032, 8) 129 row
                            blocks through col_lse_kernel. 64-row form: (64, 65, 8); (4, 1025, 8) 17 partials.
  lg_assign_matches[_lens]  (1, 1, 8), (1, 33, 72), (3, 300, 296), (1, 70, 520) on `exact` and `peaky`, thresholds 0,
                            0.1 and 1, whole and ragged: indices, counts, list and padding equal the float64
                            reference's; scores within the score bound carried through exp.
  lg_pair_inputs            rows 1, 7, 9 (n0 = 0, n1 = 0 among them) and three pairs of 9 + 7.

Every test prints its worst error / bound per input set (recorded in profiles/assignment_exact/INDEX.md).
"""
import numpy as np
import pytest
import torch

import assignment_refs as R
from gpu_common import GUARD_BYTES, SENTINEL_BYTE, GuardedIn

pytestmark = pytest.mark.gpu

F16, F32, I32 = torch.float16, torch.float32, torch.int32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def call(name, *args):
    from lightglue_amd import _host

    _host.call(name, *args, torch.cuda.current_stream().cuda_stream)


class Guarded:
    """`shape` of `dtype` inside an allocation of SENTINEL_BYTE, GUARD_BYTES of it on both sides. check(): the guards
    unchanged and (written=True) no element still the sentinel pattern -> the CPU copy. Unlike gpu_common.GuardedOut
    the region may legitimately come back NaN, and may be bytes (a workspace)."""

    def __init__(self, shape, dtype, dev):
        numel = int(np.prod(shape)) if len(shape) else 1
        es = torch.empty((), dtype=dtype).element_size()
        self.lo, self.hi = GUARD_BYTES, GUARD_BYTES + numel * es
        self.buf = torch.full((self.hi + GUARD_BYTES,), SENTINEL_BYTE, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.hi].view(dtype).view(*shape)
        self.ptr = self.buf.data_ptr() + self.lo

    def check(self, what, written=True):
        assert bool((self.buf[:self.lo] == SENTINEL_BYTE).all()), f"{what}: wrote before the buffer"
        assert bool((self.buf[self.hi:] == SENTINEL_BYTE).all()), f"{what}: wrote past the buffer"
        out = self.view.cpu()
        if written and out.numel():
            es = out.element_size()
            left = (out.contiguous().view(torch.uint8).view(-1, es) == SENTINEL_BYTE).all(1)
            assert not bool(left.any()), f"{what}: {int(left.sum())} elements not written"
        return out.numpy()


def lens_on(dev, inp):
    if inp.mlen is None:
        return None, None
    return torch.from_numpy(inp.mlen).to(dev), torch.from_numpy(inp.nlen).to(dev)


def report(title, worst):
    print(f"{title}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- lg_assign_scores / lg_assign_scores_lens -----------------------------------------------------------------------------------
def run_assign_scores(dev, lib, inp):
    pr, m, n = inp.shape
    v = GuardedIn(torch.from_numpy(inp.v), dev)
    out = Guarded((pr, m, n), F32, dev)
    ws = Guarded((lib.lg_assign_scores_workspace(m, n, pr),), torch.uint8, dev)
    ml, nl = lens_on(dev, inp)
    if ml is None:
        call("lg_assign_scores", v.ptr, (m + n) * R.LD, R.LD, R.ZC, m, n, pr, out.ptr, ws.ptr)
    else:
        call("lg_assign_scores_lens", v.ptr, (m + n) * R.LD, R.LD, R.ZC, m, n, pr, ml.data_ptr(), nl.data_ptr(), out.ptr, ws.ptr)
    torch.cuda.synchronize()
    wsb = ws.check(f"workspace {inp.kind} {inp.shape}", written=False)
    sim = wsb[:pr * m * n * 2].view(np.float16).reshape(pr, m, n)    # (the workspace's documented first region)
    return out.check(f"scores {inp.kind} {inp.shape}"), sim


def check_sim(inp, sim, x, doubt):
    """The fp16 similarity the head leaves in its workspace against fp16(float64 m0 . m1^T) on the valid block: equal
    where x is exact; elsewhere it may differ only at the elements the bound holds in doubt, by at most their dx.
    -> the number of elements that differ."""
    pr, m, n = inp.shape
    moved = 0
    for p in range(pr):
        ml, nl = (m if inp.mlen is None else int(inp.mlen[p])), (n if inp.nlen is None else int(inp.nlen[p]))
        a, b = sim[p, :ml, :nl].astype(np.float64), x[p, :ml, :nl]
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        if doubt is None:
            assert same.all(), (inp.kind, inp.shape, p, int((~same).sum()), "similarities differ from the exact ones")
        else:
            assert (same | (doubt[p, :ml, :nl] > 0)).all(), (inp.kind, inp.shape, p, "a similarity moved outside the doubt set")
            assert (np.abs(a - b) <= doubt[p, :ml, :nl])[~same].all(), (inp.kind, inp.shape, p, "moved by more than dx")
            moved += int((~same).sum())
    return moved


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


@pytest.mark.parametrize("ragged", (False, True))
@pytest.mark.parametrize("shape", sorted(R.ASSIGN_SHAPES))
def test_assign_scores_against_float64(dev, lib, shape, ragged):
    """Every input set at one shape: exact similarities (so the float64 reference is the truth), Gaussian ones, one-hot
    rows, ramps both ways, extreme matchability logits and a NaN row; whole, and ragged through the _lens entry point
    (-inf exactly on the padding, whose rows of v hold NaN and Inf)."""
    pr, m, n = shape
    worst, fails = {}, []   # (every set runs: one failing set does not hide the next)
    for kind in R.V_SETS:
        inp = R.Inputs(kind, shape, ragged)
        x, z0, z1, doubt = inp.operands()
        ref, bound = R.ref_scores(x, z0, z1, R.chain_assign(m, n, pr), inp.mlen, inp.nlen, doubt)
        got, sim = run_assign_scores(dev, lib, inp)
        moved = check_sim(inp, sim, x, doubt)
        if doubt is not None:
            print(f"{kind} {shape}: {int((doubt > 0).sum())} similarities in doubt, {moved} not the reference's fp16 value")
        worst[kind], msg = R.compare(got, ref, bound)
        if msg is not None:
            fails.append((kind, msg))
    report(f"lg_assign_scores{'_lens' if ragged else ''} {shape}", worst)
    assert not fails, (shape, ragged, fails)


# ---- lg_log_double_softmax (fp32) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.F32_SHAPES)
def test_log_double_softmax_f32_against_float64(dev, lib, shape):
    """The sets above as fp32 sim / z, and -inf entries: at the head of a thread's column walk, a whole 128-row chunk of
    them above finite rows, a row's tail; -inf exactly there and the bound elsewhere."""
    pr, m, n = shape
    worst, fails = {}, []   # (every set runs: one failing set does not hide the next)
    for kind in R.SIM_SETS:
        x, z0, z1 = R.sim_inputs(kind, shape)
        ref, bound = R.ref_scores(x, z0, z1, R.chain_f32(m, n))
        sim, a, b = (GuardedIn(torch.from_numpy(t.astype(np.float32)), dev) for t in (x, z0, z1))
        out = Guarded(shape, F32, dev)
        ws = Guarded((lib.lg_log_double_softmax_workspace(m, n, pr),), torch.uint8, dev)
        call("lg_log_double_softmax", sim.ptr, a.ptr, b.ptr, m, n, pr, out.ptr, ws.ptr)
        torch.cuda.synchronize()
        ws.check(f"workspace {kind} {shape}", written=False)
        worst[kind], msg = R.compare(out.check(f"scores {kind} {shape}"), ref, bound)
        if msg is not None:
            fails.append((kind, msg))
    report(f"lg_log_double_softmax {shape}", worst)
    assert not fails, (shape, fails)


# ---- lg_log_double_softmax_f16 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(R.F16_SHAPES))
def test_log_double_softmax_f16_against_float64(dev, lib, shape):
    """fp16 sim read directly, the logits strided (channel 3 of 8-channel rows, image 0's rows then image 1's)."""
    pr, m, n = shape
    worst, fails = {}, []   # (every set runs: one failing set does not hide the next)
    zs = 8
    for kind in R.SIM_SETS:
        x, z0, z1 = R.sim_inputs(kind, shape)
        x = x.astype(np.float16)
        ref, bound = R.ref_scores(x.astype(np.float64), z0, z1, R.chain_f16(m, n, pr))
        zrows = np.full((pr, m + n, zs), np.nan, np.float16)     # (a read of another channel shows)
        zrows[:, :m, 3], zrows[:, m:, 3] = z0, z1
        sim, z = GuardedIn(torch.from_numpy(x), dev), GuardedIn(torch.from_numpy(zrows), dev)
        out = Guarded(shape, F32, dev)
        ws = Guarded((lib.lg_log_double_softmax_f16_workspace(m, n, pr),), torch.uint8, dev)
        call("lg_log_double_softmax_f16", sim.ptr, z.ptr + 3 * 2, z.ptr + (m * zs + 3) * 2, (m + n) * zs, zs, m, n, pr, out.ptr,
             ws.ptr)
        torch.cuda.synchronize()
        ws.check(f"workspace {kind} {shape}", written=False)
        worst[kind], msg = R.compare(out.check(f"scores {kind} {shape}"), ref, bound)
        if msg is not None:
            fails.append((kind, msg))
    report(f"lg_log_double_softmax_f16 {shape}", worst)
    assert not fails, (shape, fails)


# ---- lg_assign_matches / lg_assign_matches_lens -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", (False, True))
@pytest.mark.parametrize("kind", ("exact", "peaky"))
@pytest.mark.parametrize("shape", R.MATCH_SHAPES)
def test_assign_matches_against_float64(dev, lib, shape, kind, ragged):
    """The match head against filter_matches_dense's semantics applied in float64 to the float64 scores: no row, column
    or threshold decision of these inputs lies within 16 bounds of a tie (asserted on the CPU), so every index, count,
    list row and padding entry must be equal, and every non-zero score within the bound carried through exp."""
    pr, m, n = shape
    k = min(m, n)
    inp, sc, bd = R.match_inputs(kind, shape, ragged)
    v = GuardedIn(torch.from_numpy(inp.v), dev)
    ml, nl = lens_on(dev, inp)
    worst = 0.0
    for th in R.THRESHOLDS:
        want = R.ref_matches(sc, th, inp.mlen, inp.nlen)
        outs = dict(matches0=Guarded((pr, m), I32, dev), matches1=Guarded((pr, n), I32, dev), scores0=Guarded((pr, m), F32, dev),
                    scores1=Guarded((pr, n), F32, dev), matches=Guarded((pr, k, 2), I32, dev),
                    match_scores=Guarded((pr, k), F32, dev), counts=Guarded((pr,), I32, dev))
        ws = Guarded((lib.lg_assign_matches_workspace(m, n, pr),), torch.uint8, dev)
        head = (v.ptr, (m + n) * R.LD, R.LD, R.ZC, m, n, pr)
        tail = tuple(outs[f].ptr for f in ("matches0", "matches1", "scores0", "scores1", "matches", "match_scores", "counts")) + (ws.ptr,)
        if ml is None:
            call("lg_assign_matches", *head, th, *tail)
        else:
            call("lg_assign_matches_lens", *head, ml.data_ptr(), nl.data_ptr(), th, *tail)
        torch.cuda.synchronize()
        ws.check(f"workspace {kind} {shape} th={th}", written=False)
        g = {f: o.check(f"{f} {kind} {shape} th={th}") for f, o in outs.items()}
        for f in ("matches0", "matches1", "matches", "counts"):
            assert (g[f] == want[f]).all(), (f, kind, shape, ragged, th, int((g[f] != want[f]).sum()))
        # scores: zero exactly where the reference is, else within the bound; the column side and the list copy the row side
        pi, ri = np.indices((pr, m))
        e_row = R.mscore_bound(np.nan_to_num(want["best0"]), bd[pi, ri, want["arg0"]])
        mutual0 = want["scores0"] > 0
        assert ((g["scores0"] == 0) == ~mutual0).all() and ((g["scores1"] == 0) == ~(want["scores1"] > 0)).all()
        err = np.abs(g["scores0"].astype(np.float64) - want["scores0"])
        worst = max(worst, float((err / e_row)[mutual0].max(initial=0.0)))
        assert (err <= e_row)[mutual0].all(), (kind, shape, ragged, th, worst)
        mutual1 = want["scores1"] > 0
        assert (g["scores1"][mutual1] == np.take_along_axis(g["scores0"], want["arg1"], 1)[mutual1]).all()
        for p in range(pr):
            c = int(want["counts"][p])
            assert (g["match_scores"][p, :c] == g["scores0"][p, want["matches"][p, :c, 0]]).all()
            assert (g["match_scores"][p, c:] == 0).all()
    print(f"lg_assign_matches{'_lens' if ragged else ''} {kind} {shape}: worst mscore error / bound {worst:.3f}")


# ---- lg_pair_inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1,pairs", [(1, 0, 1), (0, 7, 1), (4, 5, 1), (9, 7, 3)])
def test_pair_inputs_against_float64(dev, lib, n0, n1, pairs):
    """x bit for bit; cos / sin = the correctly rounded fp16 of float64 cos / sin of the fp16 projection, or its neighbour
    only where the float64 value lies within cosf's error (4 fp32 ulps) of an fp16 rounding boundary: those are counted,
    and the kernel may differ from the correctly rounded value at no other element."""
    rows = pairs * (n0 + n1)
    kp, wr = R.pair_inputs_operands(rows)
    proj, c64, s64, single = R.pair_inputs_ref(kp, wr)
    assert single.all()
    rng = np.random.default_rng(R.seed_of("desc", n0, n1, pairs))
    desc = rng.normal(size=(rows, 256)).astype(np.float16)
    img0 = np.concatenate([np.arange(p * (n0 + n1), p * (n0 + n1) + n0) for p in range(pairs)]).astype(np.int64)
    img1 = np.setdiff1d(np.arange(rows), img0)
    put = lambda a: GuardedIn(torch.from_numpy(np.ascontiguousarray(a)), dev) if len(a) else None  # noqa: E731
    d0, d1, k0, k1 = put(desc[img0]), put(desc[img1]), put(kp[img0]), put(kp[img1])
    w = GuardedIn(torch.from_numpy(wr), dev)
    x, co, si = Guarded((rows, 256), F16, dev), Guarded((rows, 64), F16, dev), Guarded((rows, 64), F16, dev)
    ptr = lambda t: t.ptr if t is not None else None  # noqa: E731
    call("lg_pair_inputs", ptr(d0), ptr(d1), ptr(k0), ptr(k1), w.ptr, n0, n1, pairs, 256, x.ptr, co.ptr, si.ptr)
    torch.cuda.synchronize()
    assert np.array_equal(x.check("x").view(np.uint16), desc.view(np.uint16))
    near = off = 0
    for name, got, val in (("cos", co.check("cos"), c64), ("sin", si.check("sin"), s64)):
        assert np.array_equal(got[:, 0::2].view(np.uint16), got[:, 1::2].view(np.uint16)), name   # a rotary pair shares its value
        got = got[:, 0::2]
        lo, hi = R.f16_candidates(val, 8.0 * R.U * np.abs(val) + R.TINY)
        assert ((got == lo) | (got == hi)).all(), (name, int(((got != lo) & (got != hi)).sum()))
        near += int((lo != hi).sum())
        off += int((got != val.astype(np.float16)).sum())
    assert off <= near
    print(f"lg_pair_inputs {pairs} x ({n0} + {n1}): {2 * rows * 32} values, {near} within cosf's error of an fp16 boundary, "
          f"{off} not the correctly rounded value")
