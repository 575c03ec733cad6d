"""What tests/test_gpu_attention_backward_exact.py (the kernels on the MI355X) and
tests/test_attention_backward_reference.py (operands, bounds and mutants, no GPU) share for the attention backward
(csrc/mha_hd64_backward.hip: the rows kernel, the cols kernel, the split reduce): the planner restated, operand
families on which every query and every key counts exactly once, the float64 reference, a derived elementwise bound
for graded operands, and a NumPy fp32 restatement of the three kernels whose mutants are parameters. A plain module:
numpy and ctypes only, no fixtures, nothing here touches a GPU.

The operation, per (batch, head), on the five tensors the kernel is given (q, k, v, o, dout, all fp16-exact here):
    P = softmax(Q K^T / 8),  D_i = sum_d dO_id O_id (from the SUPPLIED O, not recomputed),  dP = dO V^T,
    dS = P (dP - D),  dQ = dS K / 8,  dK = dS^T Q / 8,  dV = P^T dO.
`reference64` is exactly that in float64, everywhere in this file.

What the kernels do (read from the .hip file): x = fp32(q . k) kScaleLog2 (no fp16 rounding of the scaled query, unlike
the forward); rows: an online maximum and sum over 64-key tiles, L = M + v_log_f32(l); D as 64 fp32 products; P =
v_exp_f32(x - L); dP by MFMA in fp32; dS = P (dP - D) in fp32, rounded to fp16 ONCE as an MFMA operand; dQ accumulated
in fp32 over the keys, times 1/8. cols: P and dS again from the workspace's L and D, both rounded to fp16 once; dV +=
dO^T P16 and dK += Q^T dS16 in fp32 over the query blocks of a split, dK times 1/8; one split: stored; several: fp32
partials in the workspace, added in split order by the reduce, rounded once.

The plan (`plan_backward`, `plan_for`): qtiles, ktiles, splits, tiles_per_split and ws_bytes restated; `plan_for`
asserts ws_bytes against mha_hd64_backward_workspace_bytes every time it hands a plan out (the partial bytes pin the
split count). `seams`: the first and last query of every block and every split, the first and last key of every block.

The exact families. Every quantity the kernels round is exactly representable, which `assert_exact_conditions` checks
on the float64 reference's own P and dS before a case is used: every P and dS is an fp16 value (to within 2^-190, which
no rounding of the kernels or of the outputs can see: `GAP_MIN` = 200 log2 units between a selected key and every
other), every product that enters a sum is an integer multiple of one quantum and the sum of their magnitudes is below
2^24 quanta (so every partial sum is exact in fp32 in ANY order, across blocks, splits and the reduce), O is fp16-exact.
The one modelled constant is attention_refs.E_HW: v_exp_f32 and v_log_f32 within 2^-23 relative. With it the fp32 P is
within 2^-20 relative of 1 / nkv, 1 / |B| or 1 (L = log2 nkv <= 10 off by 10 * 2^-23, times ln 2, plus the exponential's
own 2^-23), a value whose fp16 rounding boundary is 2^-12 away; dS = P (dP - D) with dP - D exact then lies as close to
an fp16 value and rounds to it. So the check (`check_exact`) is numeric equality with the reference rounded to the
output type, on every element; -0 and +0 compare equal; no NaN anywhere. Its ratio is |got - ref| over half an output
ulp of the reference.
  census_q0  Q = 0, nkv a power of two: every P is 1 / nkv. K is a key census (attention_refs.census_v: a one-hot
             column plus index bits). V holds 0s and 1s with m_c ones in column c, 1 <= m_c <= nkv - 1, so each column
             mean m_c / nkv is fp16-exact and differs from each entry. dO rows are one-hot, scaled by small integers; O
             is the exact column mean. dV = sum_i dO_i / nkv: each query once. dQ_i = sum_j dS_ij K_j / 8 with dS != 0
             for every j: each key once. dK = 0.
  census_k0  K = 0, Q a query census: dK_j = sum_i dS_ij Q_i / 8 counts every query once across blocks and splits;
             dQ = 0.
  selector   K rows are +-1 codes, row i's query 64 code(pi(i)): P is one-hot and l = 1 in fp32. V holds integers in
             -2 .. 2, dO in -1 .. 1 and O = V[pi(i)], so dP - D is exactly 0 on the target: dQ = dK = 0, and dV_j is
             the sum of the dO rows that select j (integers: any summation order). Targets sit on the first and last
             key of every key block and on nkv - 1; the two queries on either side of every block seam and split seam
             select the same key.
  twolevel   a run B of 2 or 4 keys shares a code and straddles a key-block seam or ends at nkv - 1; V differs inside
             B and dP - D is nonzero on every key of B (asserted). P is 1 / |B| on B. dQ = code * sum_{j in B} dS_ij /
             8 = 0 only if every key of B is counted, in L and in dS alike; dK on B is 8 code sum_i dS_ij, exact.
  mixed      selector and two-level rows interleaved row by row, the order shifted per (batch, head), and a different
             code flip, V and dO per (batch, head): L and D of one head are wrong for the same row of another, and so
             are its Q and K. (The census kinds need Q = 0 or K = 0 and a power-of-two nkv and stay in their own
             cases.)

The graded families (`graded_case`, `graded_bound`): gauss1, peaked (logits to +-40) and spike (one key dominates a
row) as tools/attention_backward_host_check.py generates them, fp16-rounded, O = fp16 of the float64 forward. Each
output element is held to a bound derived term by term from the float64 magnitudes it acts on. U = 2^-24, u16 = 2^-11,
E = E_HW; n keys, T = ceil(n / 64) tiles, S splits; s_ij the exact scores in log2 units, p_ij the exact weights, g_ij =
dP_ij - D_i, dS_ij = p_ij g_ij.
  scores   dx_ij = 80 U A_ij, A_ij = sum_d |q_id k_jd| kScaleLog2: 64 products accumulated in fp32, the fp32 constant
           kScaleLog2 against log2(e) / 8 and the multiplication (66, rounded up as attention_refs does).
  subtract every x - m and x - L is one fp32 subtraction of numbers up to max_j |s_ij| and |L| <= max |s| + log2 n:
           dsub_i = U (2 max_j |s_ij| + log2 n + 1), absolute, log2 units.
  L        dL_i = log2(sum_j p_ij 2^dx_ij)                     (what the score errors can move a log-sum-exp by)
                + dsub_i                                       (x - m inside the sum)
                + ((n + 2 T + 4) U + (T + 1) (E + U) + E) / ln 2   (n additions, T rescales and the half-wave merge
                                                               with their exponentials, each term's exponential)
                + E log2 n + U (max_j |s_ij| + log2 n)         (v_log_f32 on l in [1, n], the final M + log)
  P        relative, fp32: eps_ij = (2^(dx_ij + dL_i + dsub_i) - 1) (1 + E) + E.
  dP, D    eg_ij = 64 U sum_d |dO_id v_jd| + 65 U sum_d |dO_id o_id| + U |g_ij|: the two 64-term fp32 sums (D's products
           are rounded one by one, and its half-wave add) and the subtraction.
  dS       fp32: e32_ij = |g_ij| p_ij eps_ij + p_ij (1 + eps_ij) eg_ij, plus the product's rounding U (|dS_ij| + e32_ij);
           then ONE fp16 rounding: u16 (|dS_ij| + e32_ij), or half the fp16 subnormal spacing, 2^-25: both are added.
  P16      eP_ij = p_ij eps_ij + u16 p_ij (1 + eps_ij) + 2^-25 + 2^-126 (a flushed fp32 subnormal).
  sums     dQ_id: sum_j e_dS_ij |k_jd| / 8 + (n + 8) U sum_j (|dS_ij| + e_dS_ij) |k_jd| / 8
           dK_jd: sum_i e_dS_ij |q_id| / 8 + (nq + 8 + S) U sum_i (|dS_ij| + e_dS_ij) |q_id| / 8
           dV_jd: sum_i eP_ij |dO_id| + (nq + 8 + S) U sum_i (p_ij + eP_ij) |dO_id|
           (fp32 accumulation over the contracted index, the S - 1 split adds; the factor 1 / 8 is exact)
  output   half an ulp of the output type at |ref| + bound (fp16: 2^-11 relative or 2^-25; fp32: none, the last fp32
           operation's rounding is in the sums).
Nothing is multiplied on top. A GPU figure above 1 is a rounding this derivation missed (name it, add it) or a bug.

The restatement (`restate`) and its mutants: see its docstring.
"""
import math
import os

import numpy as np

import attention_refs as R
from attention_refs import E_HW, HEAD_DIM, SCALE_LOG2, SUB16, U, U16, cdiv, f16, is_f16

BLOCK = 64                # queries per rows workgroup and per streamed block, keys per cols workgroup
GAP_MIN = 200.0           # log2 units between a selected key (or run) and every other key
HALF, FLOAT = 1, 0        # mha_hd64_dtype_t
MASKED = np.float32(-1e30)

# batch, heads, nq, nkv -> (splits, tiles_per_split) as the issue claims them (None: no claim beyond the plan itself)
SHAPES = {
    (1, 4, 1, 1): (1, 1),
    (1, 4, 63, 65): (1, 1),
    (1, 4, 65, 63): (2, 1),
    (1, 4, 130, 129): (3, 1),
    (2, 3, 70, 45): (2, 1),
    (1, 1, 1024, 64): (16, 1),       # 16 splits of one block
    (1, 1, 1089, 65): (9, 2),        # 18 blocks, 9 splits of 2
    (1, 1, 1025, 64): (9, 2),        # 17 blocks: the last split is short
    (1, 1, 2050, 64): (11, 3),       # 33 blocks, splits of 3, odd starts
    (1, 4, 313, 1024): (3, 2),       # 5 blocks over at most 4 splits
    (1, 4, 1024, 1024): (4, 4),      # the workload's plan
    (8, 4, 130, 256): (2, 2),        # the last shape that splits
    (8, 4, 130, 257): (1, 3),        # the first that does not
}
CENSUS_SHAPES = [s for s in SHAPES if s[3] & (s[3] - 1) == 0]
GRADED_SHAPES = [(1, 4, 130, 129), (1, 1, 1089, 65), (1, 4, 313, 1024)]
EXACT = ("census_q0", "census_k0", "selector", "twolevel", "mixed")
GRADED = ("gauss1", "peaked", "spike")
FORCED_SHAPE, FORCED_SPLITS = (1, 1, 2050, 64), (1, 2, 16)


def families_of(shape):
    return EXACT if shape in CENSUS_SHAPES else EXACT[2:]


# ---- the plan -------------------------------------------------------------------------------------------------------
def _align256(x):
    return (x + 255) & ~255


def plan_backward(batch, heads, nq, nkv, in_f32, forced=None):
    """plan_backward of csrc/mha_hd64_backward.hip restated. forced: MHA_HD64_BWD_SPLITS (None: the environment's)."""
    if forced is None:
        e = os.environ.get("MHA_HD64_BWD_SPLITS", "")
        forced = int(e) if e.strip().isdigit() else 0
    bh = batch * heads
    qtiles, ktiles = cdiv(nq, BLOCK), cdiv(nkv, BLOCK)
    groups = bh * ktiles
    splits = 1 if groups > 128 else min(qtiles, 16, 256 // groups)
    if forced >= 1:
        splits = min(qtiles, 16, forced)
    tps = cdiv(qtiles, splits)
    splits = cdiv(qtiles, tps)
    stats = _align256(bh * nq * 4)
    qb, kb = _align256(bh * nq * HEAD_DIM * 2), _align256(bh * nkv * HEAD_DIM * 2)
    copy = 3 * qb + 2 * kb if in_f32 else 0
    part = 2 * splits * bh * nkv * HEAD_DIM * 4 if splits > 1 else 0
    return dict(batch=batch, heads=heads, nq=nq, nkv=nkv, qtiles=qtiles, ktiles=ktiles, splits=splits,
                tiles_per_split=tps, stats_bytes=stats, copy_bytes=copy, part_bytes=part, ws_bytes=2 * stats + copy + part)


def plan_for(lib, batch, heads, nq, nkv, in_f32=False):
    """The restated plan, asserted against the library's workspace query for BOTH input types (host code; it reads
    MHA_HD64_BWD_SPLITS per call, as the restatement does)."""
    for f32 in (False, True):
        p = plan_backward(batch, heads, nq, nkv, f32)
        need = lib.mha_hd64_backward_workspace_bytes(batch, heads, nq, nkv, FLOAT if f32 else HALF)
        assert need == p["ws_bytes"], (batch, heads, nq, nkv, f32, need, p)
    return plan_backward(batch, heads, nq, nkv, in_f32)


def split_blocks(plan):
    """[(t_begin, t_end)] of every split."""
    t, q = plan["tiles_per_split"], plan["qtiles"]
    return [(s * t, min(q, (s + 1) * t)) for s in range(plan["splits"])]


def odd_multiblock_splits(plan):
    return [(a, e) for a, e in split_blocks(plan) if a % 2 == 1 and e - a > 1]


def seams(plan):
    """{'q_block' | 'q_split' | 'k_block': [(first, last), ...]}."""
    nq, nkv = plan["nq"], plan["nkv"]
    return dict(q_block=[(a, min(a + BLOCK, nq) - 1) for a in range(0, nq, BLOCK)],
                q_split=[(a * BLOCK, min(e * BLOCK, nq) - 1) for a, e in split_blocks(plan)],
                k_block=[(a, min(a + BLOCK, nkv) - 1) for a in range(0, nkv, BLOCK)])


def key_targets(plan, exclude=()):
    t = [plan["nkv"] - 1, 0] + [x for ab in seams(plan)["k_block"] for x in ab]
    out = []
    for x in t:
        if x not in out and not any(a <= x < e for a, e in exclude):
            out.append(x)
    return out or [0]


def key_runs(nkv):
    """The runs B of the two-level family, disjoint: across the first key-block seam (4 keys, or 2 at 65 keys), across
    the last one (2 keys), and the last two keys."""
    runs = []
    if nkv >= 66:
        runs.append((62, 66))
    elif nkv == 65:
        runs.append((63, 65))
    last = BLOCK * (cdiv(nkv, BLOCK) - 1)
    if last > BLOCK and last + 1 <= nkv - 2:
        runs.append((last - 1, last + 1))
    if nkv >= 2 and all(e <= nkv - 2 for _, e in runs):
        runs.append((nkv - 2, nkv))
    return runs


def seam_query_pairs(plan):
    """(a - 1, a) for the first query a > 0 of every block and every split."""
    s = seams(plan)
    return sorted({(a - 1, a) for a, _ in s["q_block"] + s["q_split"] if a > 0})


# ---- the exact families ---------------------------------------------------------------------------------------------
def census_values(nkv, head):
    """V of the census families: 0s and 1s, m_c ones in column c with 1 <= m_c <= nkv - 1 (nkv a power of two >= 2:
    j -> j (2 c + 1) + c is a bijection mod nkv); one key: a single row of ones. -> (v [nkv, 64], m [64])."""
    c = (np.arange(HEAD_DIM) + 11 * head) % HEAD_DIM
    if nkv == 1:
        return np.ones((1, HEAD_DIM), np.float32), np.ones(HEAD_DIM, np.int64)
    m = 1 + (c * 37) % (nkv - 1)
    j = np.arange(nkv)[:, None]
    v = (((j * (2 * c + 1) + c) % nkv) < m).astype(np.float32)
    assert (v.sum(0) == m).all()
    return v, m


def _ints(seed, shape, lo, hi):
    from lightglue_amd import synth

    n = int(np.prod(shape))
    return (np.floor(synth.uniform24(seed, n) * (hi - lo + 1)) + lo).astype(np.float32).reshape(shape)


def exact_case(family, plan, seed=11):
    """The five tensors of an exact family for `plan` (from plan_for): dict q, k, v, o, dout [batch, heads, n, 64]
    float32 (fp16-exact), kind [batch, heads, nq] of b'c' / b's' / b't', target and run [batch, heads, nq], runs."""
    batch, heads, nq, nkv = (plan[x] for x in ("batch", "heads", "nq", "nkv"))
    z = lambda n: np.zeros((batch, heads, n, HEAD_DIM), np.float32)
    q, k, v, o, dout = z(nq), z(nkv), z(nkv), z(nq), z(nq)
    kind = np.zeros((batch, heads, nq), "S1")
    target = np.full((batch, heads, nq), -1, np.int64)
    run_of = np.full((batch, heads, nq), -1, np.int64)
    case = dict(family=family, plan=plan, q=q, k=k, v=v, o=o, dout=dout, kind=kind, target=target, run=run_of, runs=[])
    rows = np.arange(nq)
    if family in ("census_q0", "census_k0"):
        assert nkv & (nkv - 1) == 0, "the census families need a power-of-two key count"
        amps = np.array((1, -2, 3, -1, 2, -3) if nkv <= 512 else (1, -2, 4, -1, 2, -4), np.float32)
        for b in range(batch):
            for h in range(heads):
                g = b * heads + h
                vv, m = census_values(nkv, g)
                v[b, h] = vv
                col = (rows * 5 + 3 * g) % HEAD_DIM
                dout[b, h, rows, col] = amps[(rows + g) % len(amps)]
                o[b, h] = (m / nkv).astype(np.float32)
                if family == "census_q0":
                    k[b, h] = R.census_v(nkv, g)
                else:
                    q[b, h] = R.census_v(nq, g)
        kind[:] = b"c"
    else:
        runs = key_runs(nkv) if family in ("twolevel", "mixed") else []
        case["runs"] = runs
        tg = key_targets(plan, runs)
        step = len(tg) // 2 + 1
        while math.gcd(step, len(tg)) != 1:
            step += 1
        flips = R._codes(seed * 7 + 3, batch * heads).reshape(batch, heads, HEAD_DIM)
        pairs = seam_query_pairs(plan)
        for b in range(batch):
            base, gap = R._code_table(seed * 7 + b, nkv, tuple(runs))
            gap *= 64 * SCALE_LOG2 / R.Q_TILDE      # (the backward scales fp32(q . k) by kScaleLog2, no fp16 step)
            assert gap >= GAP_MIN, f"codes: gap {gap:.1f} log2 units at {nkv} keys, seed {seed}"
            for h in range(heads):
                g = b * heads + h
                kk = base * flips[b, h]
                k[b, h] = kk
                vv = _ints(seed * 13 + 5 * g + 1, (nkv, HEAD_DIM), -2, 2)
                dd = _ints(seed * 13 + 5 * g + 2, (nq, HEAD_DIM), -1, 1)
                for a, e in runs:       # V differs inside a run
                    for j in range(a + 1, e):
                        if (vv[a:j] == vv[j]).all(1).any():
                            vv[j, j % HEAD_DIM] = -vv[j, j % HEAD_DIM] if vv[j, j % HEAD_DIM] else 1.0
                two = np.zeros(nq, bool)
                if runs:
                    two[:] = True if family == "twolevel" else (rows + g) % 2 == 1
                t = np.array(tg)[(rows * step + g) % len(tg)]
                if family == "selector":    # the same key from both sides of every query seam
                    for n, (r0, r1) in enumerate(pairs):
                        t[r0] = t[r1] = tg[(n + g) % len(tg)]
                r = (rows // (2 if family == "mixed" else 1) + g) % max(1, len(runs))
                for i in np.flatnonzero(two):       # dP - D nonzero on every key of the run
                    a, e = runs[r[i]]
                    dev = (vv[a:e] - vv[a:e].mean(0)).astype(np.float64)
                    for d in range(HEAD_DIM):
                        if (dev @ dd[i].astype(np.float64) != 0).all():
                            break
                        dd[i, d] = (dd[i, d] + 2) % 3 - 1
                    assert (dev @ dd[i].astype(np.float64) != 0).all(), (family, b, h, i)
                sel = ~two
                kind[b, h] = np.where(two, b"t", b"s")
                target[b, h, sel] = t[sel]
                run_of[b, h, two] = r[two]
                q[b, h, sel] = HEAD_DIM * kk[t[sel]]
                o[b, h, sel] = vv[t[sel]]
                if runs:
                    starts = np.array([a for a, _ in runs])
                    means = np.array([vv[a:e].astype(np.float64).mean(0) for a, e in runs])
                    q[b, h, two] = HEAD_DIM * kk[starts[r[two]]]
                    o[b, h, two] = means[r[two]].astype(np.float32)
                v[b, h] = vv
                dout[b, h] = dd
    assert all(is_f16(x) for x in (q, k, v, o, dout))
    return case


def reference64(case, b, h, parts=False):
    """(dq, dk, dv) float64 of one (batch, head): the closed form on the five tensors, D from the supplied O.
    parts: also (p, ds)."""
    q, k, v, o, do = (case[x][b, h].astype(np.float64) for x in ("q", "k", "v", "o", "dout"))
    s = (q @ k.T) * 0.125
    p = np.exp(s - s.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    d = (do * o).sum(1, keepdims=True)
    ds = p * (do @ v.T - d)
    out = (ds @ k * 0.125, ds.T @ q * 0.125, p.T @ do)
    return out + (p, ds) if parts else out


def reference_all(case, check=False):
    """The float64 (dq, dk, dv) [batch, heads, n, 64] of a case; check: assert_exact_conditions on every head."""
    plan = case["plan"]
    outs = [np.zeros(case[x].shape, np.float64) for x in ("q", "k", "v")]
    for b in range(plan["batch"]):
        for h in range(plan["heads"]):
            res = reference64(case, b, h, parts=True)
            if check:
                assert_exact_conditions(case, b, h, res)
            for dst, x in zip(outs, res[:3]):
                dst[b, h] = x
    return tuple(outs)


def _quantum(x):
    """The largest power of two of which every element of x is an integer multiple (1 for an all-zero x)."""
    x = np.abs(np.asarray(x, np.float64))
    x = x[x != 0]
    if x.size == 0:
        return 1.0
    m, e = np.frexp(x)
    mant = (m * 2.0 ** 53).astype(np.int64)
    low = np.log2((mant & -mant).astype(np.float64))
    return float(2.0 ** (e - 53 + low).min())


def assert_exact_conditions(case, b, h, res):
    """On the float64 reference's own p and ds (res = reference64(.., parts=True)): they are fp16 values to within
    2^-190; every product entering dQ, dK, dV is a multiple of one quantum with the magnitudes summing below 2^24 quanta;
    O is fp16-exact; and what each family's name promises."""
    p, ds = res[3], res[4]
    q, k, v, o, do = (case[x][b, h].astype(np.float64) for x in ("q", "k", "v", "o", "dout"))
    fam, nkv = case["family"], case["plan"]["nkv"]
    p16, ds16 = (x.astype(np.float16).astype(np.float64) for x in (p, ds))
    assert np.abs(p - p16).max() <= 2.0 ** -190 and np.abs(ds - ds16).max() <= 2.0 ** -190, (fam, b, h)
    assert is_f16(case["o"][b, h])
    for name, w, x in (("dq", ds16, k), ("dk", ds16.T, q), ("dv", p16.T, do)):
        quantum = _quantum(w) * _quantum(x)
        assert (np.abs(w) @ np.abs(x)).max() / quantum < 2.0 ** 24, (fam, name, b, h)
    if fam.startswith("census"):
        assert (p16 == 1.0 / nkv).all()
        assert nkv == 1 or (ds16 != 0).all(), "a key or query without weight"
        assert (res[1] == 0).all() if fam == "census_q0" else (res[0] == 0).all()
    else:
        kind = case["kind"][b, h]
        sel = kind == b"s"
        assert ((p16[sel] == 1).sum(1) == 1).all() and ((p16[sel] != 0).sum(1) == 1).all()
        assert (ds16[sel] == 0).all()
        for n, (a, e) in enumerate(case["runs"]):
            rows = (kind == b"t") & (case["run"][b, h] == n)
            assert (p16[rows][:, a:e] == 1.0 / (e - a)).all() and (p16[rows].sum(1) == 1).all()
            assert (ds16[rows][:, a:e] != 0).all() and (ds16[rows].sum(1) == 0).all()
        assert (np.abs(res[0]) <= 2.0 ** -150).all()


def round_out(x, out16):
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16 if out16 else np.float32)


def check_exact(got, ref, out16, what=""):
    """got against the float64 ref of an exact family: numeric equality with the reference rounded to the output type
    on every element, no NaN -> worst |got - ref| over half an output ulp of the reference (at most 1 when equal)."""
    got = np.asarray(got)
    assert got.dtype == (np.float16 if out16 else np.float32), got.dtype
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} NaN (an element not written, or poison read)"
    want = round_out(ref, out16)
    assert np.isfinite(want).all()
    if not (got == want).all():
        bad = np.argwhere(got != want)
        at = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} elements differ from the rounded reference, first at {at}: got "
                             f"{float(got[at])!r}, reference {float(ref[at])!r}")
    half_ulp = 0.5 * np.spacing(np.abs(want)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    return float(np.where(err == 0, 0.0, err / half_ulp).max())


# ---- the graded families --------------------------------------------------------------------------------------------
def graded_case(name, plan, seed=5):
    """gauss1 / peaked / spike as tools/attention_backward_host_check.py builds them, fp16-rounded, O = fp16 of the
    float64 forward on them."""
    from lightglue_amd import synth

    batch, heads, nq, nkv = (plan[x] for x in ("batch", "heads", "nq", "nkv"))
    q, k, v = synth.qkv(seed, nq, nkv, q_std=10.0 if name == "peaked" else 1.0, batch=batch, heads=heads)
    if name == "spike":
        k = synth.spike(q, k, nq // 2, max(0, nkv - 3), 4.0)
    dout = synth.normal(seed * 3 + 100, q.shape, 1.0)
    q, k, v, dout = (f16(x) for x in (q, k, v, dout))
    o, _ = R.softmax64(q, k, v)
    return dict(family=name, plan=plan, q=q, k=k, v=v, o=f16(o), dout=dout)


def graded_bound(case, b, h, out16):
    """((dq, dk, dv), (their bounds)) float64 of one (batch, head): the module docstring's bound, term by term."""
    q, k, v, o, do = (case[x][b, h].astype(np.float64) for x in ("q", "k", "v", "o", "dout"))
    nq, n = q.shape[0], k.shape[0]
    S, T = case["plan"]["splits"], cdiv(n, BLOCK)
    ln2 = math.log(2.0)
    s = R.scores64(q, k)
    p = np.exp2(s - s.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    aq, ak, av, ado = np.abs(q), np.abs(k), np.abs(v), np.abs(do)
    dx = 80 * U * (aq @ ak.T) * SCALE_LOG2
    smax, logn = np.abs(s).max(1, keepdims=True), math.log2(n)
    dsub = U * (2 * smax + logn + 1)
    dl = np.log2((p * np.exp2(dx)).sum(1, keepdims=True)) + dsub \
        + ((n + 2 * T + 4) * U + (T + 1) * (E_HW + U) + E_HW) / ln2 + E_HW * logn + U * (smax + logn)
    eps = np.expm1(ln2 * (dx + dl + dsub)) * (1 + E_HW) + E_HW
    g = do @ v.T - (do * o).sum(1, keepdims=True)
    eg = 64 * U * (ado @ av.T) + 65 * U * (ado * np.abs(o)).sum(1, keepdims=True) + U * np.abs(g)
    ds = p * g
    e32 = np.abs(g) * p * eps + p * (1 + eps) * eg
    e32 = e32 + U * (np.abs(ds) + e32)
    e_ds = e32 + U16 * (np.abs(ds) + e32) + SUB16
    e_p = p * eps + U16 * p * (1 + eps) + SUB16 + 2.0 ** -126
    mag = np.abs(ds) + e_ds
    refs = (ds @ k * 0.125, ds.T @ q * 0.125, p.T @ do)
    bounds = ((e_ds @ ak + (n + 8) * U * (mag @ ak)) * 0.125,
              (e_ds.T @ aq + (nq + 8 + S) * U * (mag.T @ aq)) * 0.125,
              e_p.T @ ado + (nq + 8 + S) * U * ((p + e_p).T @ ado))
    return refs, tuple(x + R.out_rounding(np.abs(r) + x, out16) for r, x in zip(refs, bounds))


def check_graded(got, ref, bound, what=""):
    got = np.asarray(got).astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: NaN or Inf in the output"
    ratio = np.abs(got - ref) / bound
    worst = float(ratio.max())
    if not worst <= 1.0:
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: element {at}: |got - ref| = {abs(got[at] - ref[at]):.3e} > bound {bound[at]:.3e} "
                             f"(ratio {worst:.3g})")
    return worst


# ---- the restatement ------------------------------------------------------------------------------------------------
MUTANTS = ("drop_last_key", "drop_last_query", "drop_split_first", "double_block", "reduce_omits_last", "stage_parity",
           "tail_in_L", "head0_stats", "no_D", "eighth_twice", "kv_shift")


def restate(case, out16, mutant=None, at=None, plan=None):
    """The three kernels in NumPy fp32 on a case (all heads) -> (dq, dk, dv) in the output type (out16 changes the last
    rounding only: the fp16 result is the fp32 result rounded). plan: default the case's. Rows: L by an online maximum and sum over 64-key tiles, D, then P = exp2(x - L), dS = fp16(P (dP - D)), dQ.
    Cols: per split and per head P16 and dS16 from the stored L and D, the split's query blocks contracted in fp32;
    the reduce adds the partials in split order.
    mutant:
      drop_last_key      the rows kernel masks key nkv - 1 (in L and in dS)
      drop_last_query    the cols kernel masks query nq - 1
      drop_split_first   split `at` (default the last) skips its first block
      double_block       split `at` (default 0) also visits the next split's first block (needs 2 splits)
      reduce_omits_last  the reduce leaves the last partial out (needs 2 splits)
      stage_parity       the cols kernel picks its LDS stage by t & 1, not (t - t_begin) & 1: in a split of more than
                         one block that starts at an odd block, iteration t reads the stage that holds block t - 1 (the
                         first one an unwritten stage: zeros, which add nothing), so the split's last block is lost and
                         the others are taken under their neighbour's tail mask
      tail_in_L          the masked keys of the last tile enter L with score 0
      head0_stats        the cols kernel reads L and D of (batch 0, head 0)
      no_D               D is left out (both kernels)
      eighth_twice       the 1 / 8 is applied twice (dQ and dK)
      kv_shift           K row j meets V row j + 1 in key block `at` (default the last block with two keys)"""
    f32 = np.float32
    plan = plan or case["plan"]
    batch, heads, nq, nkv = (plan[x] for x in ("batch", "heads", "nq", "nkv"))
    bh = batch * heads
    q, k, v, o, do = (case[x].reshape(bh, -1, HEAD_DIM).astype(f32) for x in ("q", "k", "v", "o", "dout"))
    scale = f32(SCALE_LOG2)
    eighth = f32(0.125 * 0.125) if mutant == "eighth_twice" else f32(0.125)
    blocks = split_blocks(plan)
    vx = v
    if mutant == "kv_shift":
        if at is None:
            at = max([t for t in range(plan["ktiles"]) if min(nkv, BLOCK * (t + 1)) - BLOCK * t >= 2], default=0)
        a, e = BLOCK * at, min(nkv, BLOCK * (at + 1))
        vx = v.copy()
        vx[:, a:e] = v[:, np.minimum(np.arange(a, e) + 1, nkv - 1)]
    lse, delta = np.zeros((bh, nq), f32), np.zeros((bh, nq), f32)
    xs, dps = [], []    # (both kernels compute the same fp32 scores and dP)
    dq = np.zeros((bh, nq, HEAD_DIM), f32)
    live = np.ones(nkv, bool)
    if mutant == "drop_last_key":
        live[nkv - 1] = False
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for g in range(bh):
            x = (q[g] @ k[g].T).astype(f32) * scale
            dp = (do[g] @ vx[g].T).astype(f32)
            xs.append(x)
            dps.append(dp)
            m, l = np.full(nq, MASKED, f32), np.zeros(nq, f32)
            for a in range(0, nkv, BLOCK):
                e = min(a + BLOCK, nkv)
                xt = x[:, a:e][:, live[a:e]]
                if mutant == "tail_in_L" and e - a < BLOCK:
                    xt = np.concatenate([xt, np.zeros((nq, BLOCK - (e - a)), f32)], 1)
                if xt.shape[1] == 0:
                    continue
                m_new = np.maximum(m, xt.max(1))
                l = l * np.exp2(m - m_new).astype(f32) + np.exp2(xt - m_new[:, None]).astype(f32).sum(1, dtype=f32)
                m = m_new
            lse[g] = m + np.log2(l).astype(f32)
            if mutant != "no_D":
                delta[g] = (do[g] * o[g]).sum(1, dtype=f32)
            p = np.exp2(x - lse[g][:, None]).astype(f32) * live
            dsr = f16(p * (dp - delta[g][:, None]))
            dq[g] = (dsr @ k[g]).astype(f32) * eighth
        S = len(blocks)
        part = np.zeros((2, S, bh, nkv, HEAD_DIM), f32)
        for g in range(bh):
            st = 0 if mutant == "head0_stats" else g
            p = np.exp2(xs[g] - lse[st][:, None]).astype(f32)
            if mutant == "drop_last_query":
                p[nq - 1] = 0
            ds16 = f16(p * (dps[g] - delta[st][:, None]))
            p16 = f16(p)
            for s, (tb, te) in enumerate(blocks):
                ts = list(range(tb, te))
                if mutant == "drop_split_first" and s == (S - 1 if at is None else at):
                    ts = ts[1:]
                if mutant == "double_block" and s == (0 if at is None else at) and te < plan["qtiles"]:
                    ts.append(te)
                pairs = [(t, t) for t in ts]            # (block whose data is read, block whose tail mask applies)
                if mutant == "stage_parity" and tb % 2 == 1 and te - tb > 1:
                    pairs = [(t - 1, t) for t in ts[1:]]
                rows = [np.arange(BLOCK * d, min(nq, BLOCK * d + BLOCK))[:max(0, min(nq, BLOCK * t + BLOCK) - BLOCK * t)]
                        for d, t in pairs]
                rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
                part[0, s, g] = (ds16[rows].T @ q[g][rows]).astype(f32) * eighth
                part[1, s, g] = (p16[rows].T @ do[g][rows]).astype(f32)
        acc = part[:, 0].copy()
        for s in range(1, S - 1 if mutant == "reduce_omits_last" else S):
            acc += part[:, s]
        shape = (batch, heads, -1, HEAD_DIM)
        return tuple(round_out(x.reshape(shape), out16) for x in (dq, acc[0], acc[1]))


# ---- cases and their references, computed once ----------------------------------------------------------------------
_CASES = {}


def case_and_reference(lib, family, shape):
    """(case, (dq, dk, dv) float64) of a family at a shape under the plan in force (plan_for: asserted against the
    library); exact families have their conditions asserted here, before anything uses the case. Kept per (family,
    shape, split count): the reference is computed once and shared, and must be left unchanged."""
    plan = plan_for(lib, *shape)
    key = (family, shape, plan["splits"])
    if key not in _CASES:
        if family in EXACT:
            case = exact_case(family, plan)
            ref = reference_all(case, check=True)
        else:
            case = graded_case(family, plan)
            ref = None      # (graded_bound returns it with the bound)
        _CASES[key] = (case, ref)
    return _CASES[key]
