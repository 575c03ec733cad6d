"""What tests/test_gpu_attention_exact.py (the kernels on the MI355X) and tests/test_attention_reference.py (the
operands, the bounds and their mutants, no GPU) share for the attention family (csrc/mha_hd64_ring.hip, _direct.hip,
_direct16.hip, _stream.hip and the split combine): operand families on which every key counts exactly once, their
float64 references, the bounds, how a plan lays keys out over splits, waves, passes and tiles, and a NumPy fp32
restatement of the kernels' arithmetic whose mutants are parameters. A plain module: numpy and ctypes only, no
fixtures, nothing here touches a GPU or reads anything but its arguments.

The operation: O = softmax(Q K^T / 8) V per (batch, head), head dim 64, over keys 0 .. count - 1. Every operand here is
exactly representable in fp16, so the fp16-input and the fp32-input paths see the same numbers.

What the kernels do with them (read from the .hip files): q~ = fp16(fp32(q) * kScaleLog2); scores s = q~ . k in fp32
(log2 units); a running maximum m per row that is set exactly by a slice's first tile and afterwards moves only when
some row of the wave exceeds it by more than kRescaleThr = 8 (then every row moves to its own maximum); P = fp16(exp2(s
- m)); the row sum and P V both from that fp16 P, in fp32; the key slices of the waves of a workgroup merged in fp32
with weights exp2(m_w - M); split partials O^_s = O_s / l_s stored in the output type and merged with split_weight =
l_s * exp2(m_s - M); one product with 1 / l; the output rounding.

The exact families (no modelled term in their bounds)
  census     Q = 0: every score is 0, every P exactly 1, l the number of keys the row may see and O the column means of
             V over them. V is a key census of 0s and 1s: column (j + 7 head) mod 48 is 1 for key j, columns 48 .. 62
             hold the bits of j div 48, column 63 is the constant 1. Every partial sum is an integer below 2^24: exact
             in fp32 in any order.
  selector   K rows are +-1 codes, row i's query is 64 code(pi(i)): scores are integer multiples of q~ = fp16(64
             kScaleLog2) = 11.5390625, the target scores 738.5, and every other key trails by at least GAP_MIN = 150
             log2 units (asserted), so its P is 0 in fp16, a rescale factor past it is 0 in fp32 (2^-150 is below the
             smallest subnormal) and so is a split weight: l = 1 and O[i] = V[pi(i)] bit for bit. V is Gaussian fp16
             with 65504, the smallest normal and subnormals planted in target rows, and no negative zero.
  two-level  selector rows whose target code is shared by a run B of keys: O is the exact mean of the census V over B.
  mixed      the three kinds interleaved row by row, so the wave-wide rescale decision meets rows that disagree.
Their bound, `exact_bound`: bitwise equality on selector rows; on census and two-level rows
      (6 + S) U |ref|   S splits: O_s * (1/l_s) (1/l_s within one ulp, the product half an ulp: 3 U), w_s O^_s (U),
                        S - 1 additions (U each), the last 1 / L and product (3 U); the sums themselves are exact
    + the output rounding: half an fp16 ulp of what is rounded (2^-11 relative, 2^-25 in the subnormal range), or none
    + for split plans with fp16 output the partials' rounding: sum_s (w_s / L) 2^-11 |O^_s| = 2^-11 |ref| for V >= 0.

The graded families (`graded_bound`, elementwise against the float64 softmax on the same operands, every row):
gauss1 / gauss3 the suite's Gaussian operands at logit scales 1 and 3; lazy7, whose per-row maximum rises tile by tile
by less than 8 log2 units in all (P exceeds 1, no rescale); lazy8p, where one tile lifts it by just over 8.
With p_j the exact weights, o the exact output, U = 2^-24, u16 = 2^-11, and E the one modelled constant, the relative
error of a hardware v_exp_f32 / v_rcp_f32, E = 2^-23 (one ulp, as the CDNA ISA guide states for both):
  scores   ds_j = u16 A_j + 80 U A_j + 2^-21 (max |s| + 8),  A_j = sum_d |q_d kScaleLog2 k_jd|
           (u16 A_j: the fp16 rounding of q~, which the float64 reference does not make; 80 U A_j: 64 products and the
           bias step accumulated in fp32, the fp32 constant kScaleLog2 against log2(e) / 8; the last term: the running
           maximum enters as an fp16 pair (hi, lo), 2^-22 relative, and the subtractions)
  P        every weight, relative: eps_j = expm1(ln 2 ds_j) + R u16 + 2 E. R = 1: the fp16 rounding of P. R = 3 for the
           single-pass kernels, whose first tile's P is multiplied in fp16 by an fp16 rescale factor (two more
           roundings). The weight appears in numerator and denominator, so what reaches the output is
               T1 = sum_j p_j eps_j |v_j - o|     (not sum_j p_j |v_j|)
  floor    a P below 2^-14 relative to its (stale) maximum is an fp16 subnormal, off by up to 2^-25 absolute. The
           stale maximum lies at most F above the row's true maximum (F = 8 for the streaming kernel, which starts from
           m = 0 when all tile-0 maxima lie within +-8; else 0), so with W = sum_j 2^(s_j - smax - F):
               T2 = 2^-25 sum_j |v_j - o| / W
  both over the perturbed denominator: (T1 + T2) / (1 - max eps - 2^-25 n / W)
  sums     fp32 accumulation of P V and of l over n keys, the wave and split merges: (n + 32) U (sum_j p_j |v_j| + |o|)
  1 / l    the reciprocal and the product: (2 E + U) |o|
  output   as above; split partials with fp16 output: 2^-11 sum_s |sum_{j in s} p_j v_j| + 2^-25.
Nothing is multiplied on top.
"""
import ctypes
import math

import numpy as np

HEAD_DIM = 64
TILE = 64
SCALE_LOG2 = float(np.float32(0.18033688011112042))   # kScaleLog2, the fp32 constant of mha_hd64_device.h
RESCALE_THR = 8.0                                     # kRescaleThr
U = 2.0 ** -24
U16 = 2.0 ** -11
SUB16 = 2.0 ** -25        # half the spacing of fp16 subnormals
E_HW = 2.0 ** -23         # the modelled constant: one fp32 ulp for v_exp_f32 and v_rcp_f32
GAP_MIN = 150.0           # log2 units between a selector target and every other key
ONEHOT = 48
Q_ROWS = (1, 17, 33, 130)
WG_SHAPES = [(4, 1), (2, 2), (1, 2), (4, 2), (12, 2), (2, 4), (1, 4), (1, 8)]
RING_KEYS = (1, 63, 64, 65, 129, 257, 1000)
ONE_PASS_KEYS = (1, 64, 65, 513, 600, 1024)
TWO_PASS_KEYS = (1025, 1100, 2048)
FOUR_PASS_KEYS = (1100, 2048)
STREAM_CASE = (5, 257, 200, [200, 129, 128, 64, 65])   # test_gpu_ragged.py's "5x257x200"

GROUPS = [[(1, 130, 257), (1, 33, 1000), (2, 17, 65), (1, 1, 1)],          # one round: a single-pass kernel
          [(1, 130, 1100), (1, 33, 2048), (1, 17, 1025), (1, 1, 2048)],    # its two-pass form
          [(1, 33, 4500), (1, 130, 257), (1, 17, 1000), (1, 1, 129)]]      # past 2048 keys: a ring plan with splits
DEFAULT_SHAPES = [(1, 1, 1), (1, 17, 64), (1, 33, 65), (1, 130, 513), (1, 130, 1024), (1, 33, 1025), (1, 130, 2048),
                  (1, 17, 4500), (3, 130, 600), (2, 1056, 1100)]
GRADED_FORMS = [  # (q_waves, kv_waves, splits, nq, nkv)
    (4, 1, 1, 33, 1000), (2, 2, 3, 130, 1000), (12, 2, 2, 33, 257), (4, 2, 4, 130, 1000), (1, 2, 2, 17, 257),
    (1, 8, 0, 17, 1000), (1, 4, 0, 33, 1000), (2, 4, 0, 130, 600),
    (22, 0, 0, 33, 1024), (22, 0, 0, 130, 2048), (22, 0, 0, 17, 600), (21, 0, 0, 130, 2048), (21, 0, 0, 33, 1024),
    (21, 0, 0, 17, 600), (23, 4, 0, 130, 257), (23, 8, 0, 33, 200), (23, 4, 0, 130, 2048)]


def f16(x):
    """fp32 -> fp16 (round to nearest even) -> fp32."""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def is_f16(x):
    x = np.asarray(x)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(x.astype(np.float16).astype(x.dtype), x, equal_nan=True))


def cdiv(a, b):
    return -(-a // b)


# ---- how a plan lays the keys out -----------------------------------------------------------------------------------
def plan_of(lib, batch, heads, nq, nkv, q_waves=0, kv_waves=0, splits=0, in_f32=0, ws_bytes=64 << 20):
    """mha_hd64_plan_route of one call with forced fields as mha_hd64_launch_forced takes them ->
    dict(route, code, kv_waves, rows_per_wave, direct_tiles, splits, tiles_per_split, blocks)."""
    from lightglue_amd._lib import CallDesc

    call = (CallDesc * 1)(CallDesc(None, None, None, None, batch, heads, nq, nkv))
    out5 = (ctypes.c_int32 * 5)()
    sp, tp = (ctypes.c_int32 * 1)(), (ctypes.c_int32 * 1)()
    off = (ctypes.c_size_t * 1)()
    need = lib.mha_hd64_plan_route(call, 1, 0 if in_f32 else 1, ws_bytes, 1, q_waves, kv_waves, splits, out5, sp, tp, off)
    assert need != ctypes.c_size_t(-1).value, "mha_hd64_plan_route: bad arguments"
    rows = 16 if out5[3] == 16 else 32
    return dict(route=out5[0], code=out5[1], kv_waves=out5[2], rows_per_wave=out5[3], direct_tiles=out5[4],
                splits=sp[0], tiles_per_split=tp[0], blocks=batch * heads * cdiv(nq, rows))


def ring_forms(lib, nq, keys=RING_KEYS, heads=4):
    """Every (q_waves, kv_waves, splits) of WG_SHAPES x {1, 2, 3, 5} that the planner realises as asked at nq x nkv ->
    [(nkv, q_waves, kv_waves, splits to force, plan)], each plan once."""
    out, seen = [], set()
    for nkv in keys:
        for qw, kw in WG_SHAPES:
            for sp in (1, 2, 3, 5):
                if kw >= 4 and sp != 1:
                    continue    # one split per super-tile, whatever is asked
                plan = plan_of(lib, 1, heads, nq, nkv, qw, kw, sp)
                if plan["code"] != qw or plan["kv_waves"] != kw or (kw < 4 and plan["splits"] != sp):
                    continue
                key = (nkv, qw, kw, plan["splits"], plan["tiles_per_split"])
                if key not in seen:
                    seen.add(key)
                    out.append((nkv, qw, kw, sp, plan))
    return out


def group_plan(lib, shapes, in_f32, heads=4):
    """mha_hd64_plan_route of up to four calls [(batch, nq, nkv)] in one launch, the planner's choice -> one plan dict
    per call (as plan_of; blocks: the launch's)."""
    from lightglue_amd._lib import CallDesc

    n = len(shapes)
    calls = (CallDesc * n)(*[CallDesc(None, None, None, None, b, heads, nq, nkv) for b, nq, nkv in shapes])
    out5 = (ctypes.c_int32 * 5)()
    sp, tp = (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)()
    off = (ctypes.c_size_t * n)()
    need = lib.mha_hd64_plan_route(calls, n, 0 if in_f32 else 1, 1 << 30, 1, 0, 0, 0, out5, sp, tp, off)
    assert need != ctypes.c_size_t(-1).value
    rows = 16 if out5[3] == 16 else 32
    blocks = sum(b * heads * cdiv(nq, rows) for b, nq, _ in shapes)
    return [dict(route=out5[0], code=out5[1], kv_waves=out5[2], rows_per_wave=out5[3], direct_tiles=out5[4],
                 splits=sp[i], tiles_per_split=tp[i], blocks=blocks) for i in range(n)]


def direct_form(code, direct_tiles, blocks):
    """(waves, tiles per wave and pass, passes) of the single-pass kernels' form for a launch, as launch_direct /
    launch_direct16 choose it (4-wave forms, concurrency hint 1)."""
    if code == 22:
        return (4, 2, 1) if direct_tiles == 1 else (4, 4, 1) if direct_tiles == 2 else (4, 4, 2)
    many = blocks > 256
    if direct_tiles == 1:
        return (4, 2, 1)
    if direct_tiles == 2:
        return (4, 2, 2) if many else (4, 4, 1)
    return (4, 2, 4) if many else (4, 4, 2)


def plan_layout(plan, nkv):
    """layout[split][wave][pass] = [(a, b), ...]: the 64-key tiles, in walking order, that one wave scores under one
    rescale decision, clipped to nkv (empty ones dropped, so are waves and splits left without keys).
    Ring plans (codes 1, 2, 4, 12): split s owns super-tiles of 64 kv_waves keys, wave w tile w of each, one decision
    per tile. Single-pass kernels (21, 22): wave w owns keys from w * 64 * tiles * passes on. Streaming kernel (23):
    every wave walks all tiles."""
    def tile(a):
        return (a, min(a + TILE, nkv))

    code = plan["code"]
    if code in (21, 22):
        kw, tpw, passes = direct_form(code, plan["direct_tiles"], plan["blocks"])
        waves = []
        for w in range(kw):
            key0 = w * TILE * tpw * passes
            ps = [[tile(key0 + TILE * (p * tpw + t)) for t in range(tpw) if key0 + TILE * (p * tpw + t) < nkv]
                  for p in range(passes)]
            ps = [p for p in ps if p]
            if ps:
                waves.append(ps)
        return [waves]
    if code == 23:
        return [[[[tile(a)] for a in range(0, nkv, TILE)]]]
    kw, tps = plan["kv_waves"], plan["tiles_per_split"]
    sup = TILE * kw
    total = max(1, cdiv(nkv, sup))
    layout = []
    for s in range(plan["splits"]):
        waves = []
        for w in range(kw):
            ps = [[tile(st * sup + w * TILE)] for st in range(s * tps, min(total, (s + 1) * tps))
                  if st * sup + w * TILE < nkv]
            if ps:
                waves.append(ps)
        if waves:
            layout.append(waves)
    return layout


def layout_units(layout):
    """{'split' | 'wave' | 'pass' | 'tile': [(first key, last key), ...]} (a wave of a ring plan owns several
    stretches: each of its tiles counts as one)."""
    units = {"split": [], "wave": [], "pass": [], "tile": []}
    for waves in layout:
        keys = [t for w in waves for p in w for t in p]
        units["split"].append((min(a for a, _ in keys), max(b for _, b in keys) - 1))
        for w in waves:
            tiles = [t for p in w for t in p]
            contiguous = all(tiles[i][1] == tiles[i + 1][0] for i in range(len(tiles) - 1))
            if contiguous:
                units["wave"].append((tiles[0][0], tiles[-1][1] - 1))
            else:
                units["wave"] += [(a, b - 1) for a, b in tiles]
            for p in w:
                units["pass"].append((p[0][0], p[-1][1] - 1))
                units["tile"] += [(a, b - 1) for a, b in p]
    return units


def split_ranges(layout):
    """[(a, b)] of each split (a split of a ring plan is one stretch of keys)."""
    return [(a, b + 1) for a, b in layout_units(layout)["split"]]


def count_keys(layout, nkv):
    """How often the layout visits each key (a layout that is right visits every key once)."""
    c = np.zeros(nkv, np.int64)
    for waves in layout:
        for w in waves:
            for p in w:
                for a, b in p:
                    c[a:b] += 1
    return c


# ---- the exact families ---------------------------------------------------------------------------------------------
def census_v(nkv, head=0):
    v = np.zeros((nkv, HEAD_DIM), np.float32)
    j = np.arange(nkv)
    v[j, (j + 7 * head) % ONEHOT] = 1.0
    hi = j // ONEHOT
    for b in range(HEAD_DIM - 1 - ONEHOT):
        v[:, ONEHOT + b] = (hi >> b) & 1
    v[:, HEAD_DIM - 1] = 1.0
    return v


def _codes(seed, n):
    from lightglue_amd import synth

    return np.where(synth.uniform24(seed, n * HEAD_DIM).reshape(n, HEAD_DIM) < 0.5, -1.0, 1.0).astype(np.float32)


Q_TILDE = float(f16(np.float32(64.0) * np.float32(SCALE_LOG2)))   # 11.5390625


def code_gap(k, group):
    """Smallest distance, in log2 units after the scale, between the score of a query 64 * k[j] on key j and on any
    key of another group (keys of one group share a code)."""
    g = k @ k.T
    g[group[:, None] == group[None, :]] = -HEAD_DIM
    return float((HEAD_DIM - g.max()) * Q_TILDE) if len(k) > 1 and (group != group[0]).any() else math.inf


_TABLES = {}


def _code_table(seed, n, runs):
    """(codes [n, 64] with every run sharing its first key's code, their gap); kept: the plans of one shape share it."""
    key = (seed, n, runs)
    if key not in _TABLES:
        if len(_TABLES) > 64:
            _TABLES.clear()
        base = _codes(seed, n)
        group = np.arange(n)
        for a, e in runs:
            base[a:e] = base[a]
            group[a:e] = a
        _TABLES[key] = (base, code_gap(base, group))
    base, gap = _TABLES[key]
    return base.copy(), gap


def seam_targets(n, units):
    """Keys 0, 63, 64, 65 and n - 1, then the first and last key of every split, pass, wave and tile: below n, each
    once, in that order of priority."""
    t = [n - 1, 0, 63, 64, 65]
    for kind in ("split", "pass", "wave", "tile"):
        for a, b in units[kind]:
            t += [a, b]
    seen, out = set(), []
    for x in t:
        if 0 <= x < n and x not in seen:
            seen.add(x)
            out.append(x)
    return out


def seam_runs(n, units):
    """The runs B of the two-level family as {name: (a, b)}: `tile` straddles the first tile seam, `split` the first
    split seam (or, in a plan without one, the first pass or wave seam), `last` lies wholly in the last split (pass,
    wave) and `first` wholly in the first. Disjoint; a run that does not fit n is left out."""
    runs = {}
    if n == 1:
        return {"first": (0, 1)}
    seam = None
    for kind in ("split", "pass", "wave"):
        firsts = sorted(a for a, _ in units[kind] if a > 0)
        if firsts:
            seam, last_a = firsts[0], firsts[-1]
            break
    if n > TILE + 2:
        runs["tile"] = (TILE - 2, TILE + 2)
    if seam is not None and seam != TILE and seam + 1 <= n:
        runs["split"] = (seam - 2, min(seam + 2, n))
    lo = max([last_a if seam is not None else 0] + [b for _, b in runs.values()])
    if n - lo >= 1:
        runs["last"] = (max(lo, n - 3), n)
    first_end = min([seam if seam is not None else n, TILE, n] + [a for a, _ in runs.values()])
    if first_end >= 3:
        runs["first"] = (1, min(4, first_end))
    return runs


def exact_case(family, nq, nkv, units, seed, batch=1, heads=4, counts=None, q_counts=None):
    """One launch's operands of an exact family ('census', 'selector', 'twolevel', 'mixed') for a plan with the seams
    `units` (layout_units): dict q, k, v [batch, heads, n, 64] float32 (fp16-exact), ref float64, kind [batch, heads,
    nq] of b'c' / b's' / b't' / b'p' (a row past its query count: NaN), target [batch, heads, nq] (selector rows) and
    run [batch, heads, nq] (index into runs, two-level rows), targets, runs, gap.
    counts: per-item key counts as the kernel clamps them (into [1, nkv]); keys past a count are poison: NaN in V and
    codes that would win a row in K. units may be a function of the item's count (the seams move with it)."""
    from lightglue_amd import synth

    q = np.zeros((batch, heads, nq, HEAD_DIM), np.float32)
    k = np.zeros((batch, heads, nkv, HEAD_DIM), np.float32)
    v = np.zeros((batch, heads, nkv, HEAD_DIM), np.float32)
    ref = np.zeros((batch, heads, nq, HEAD_DIM), np.float64)
    kind = np.zeros((batch, heads, nq), "S1")
    target = np.full((batch, heads, nq), -1, np.int64)
    run_of = np.full((batch, heads, nq), -1, np.int64)
    out = dict(q=q, k=k, v=v, ref=ref, kind=kind, target=target, run=run_of, targets=[], runs=[], gap=math.inf,
               counts=[])
    flips = _codes(seed * 7 + 3, batch * heads).reshape(batch, heads, HEAD_DIM)
    for b in range(batch):
        n = nkv if counts is None else min(max(int(counts[b]), 1), nkv)
        nrows = nq if q_counts is None else min(max(int(q_counts[b]), 0), nq)
        un = units(n) if callable(units) else units
        runs = seam_runs(n, un) if family in ("twolevel", "mixed") else {}
        in_run = np.zeros(n, bool)
        for a, e in runs.values():
            in_run[a:e] = True
        tg = [t for t in seam_targets(n, un) if not in_run[t]] or [0]
        base, gap = _code_table(seed * 7 + b, n, tuple(sorted(runs.values())))
        assert gap >= GAP_MIN, f"selector codes: gap {gap:.1f} log2 units at {n} keys, seed {seed}"
        out["gap"] = min(out["gap"], gap)
        out["targets"].append(tg)
        out["runs"].append(runs)
        out["counts"].append(n)
        rl = list(runs.values())
        tgs = tg[:max(1, min(len(tg), heads * nq))]   # fewer rows than targets: the first ones, by priority
        step = len(tgs) // 2 + 1
        while math.gcd(step, len(tgs)) != 1:
            step += 1
        for h in range(heads):
            kk = base * flips[b, h]
            k[b, h, :n] = kk
            if family == "selector":
                vv = f16(synth.normal(seed * 7 + 11 * b + h + 1, (n, HEAD_DIM)))
                vv[vv == 0] = 0.0   # no negative zero
                ext = (65504.0, 2.0 ** -14, 2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, -65504.0, -2.0 ** -14, -2.0 ** -24)
                for i, t in enumerate(tg[:8]):
                    vv[t, 8 * ((i + h) % 8):8 * ((i + h) % 8) + 8] = ext
            else:
                vv = census_v(n, h)
            v[b, h, :n] = vv
            if n < nkv:   # poison: codes that win a row, NaN values
                k[b, h, n:] = kk[np.array(tg)[np.arange(nkv - n) % len(tg)]]
                v[b, h, n:] = np.nan
            v64 = vv.astype(np.float64)
            census_ref = v64.sum(0) / n
            run_ref = [v64[a:e].sum(0) / (e - a) for a, e in rl]
            g = (b * heads + h) * nq + np.arange(nq)
            kd = {"census": 0, "selector": 1, "twolevel": 2}.get(family, g % 3) * np.ones(nq, np.int64)
            if not rl:
                kd[kd == 2] = 1
            kd[np.arange(nq) >= nrows] = 3
            kind[b, h] = np.array([b"c", b"s", b"t", b"p"])[kd]
            ref[b, h, kd == 0] = census_ref
            t = np.array(tgs)[(g * step) % len(tgs)]
            target[b, h, kd == 1] = t[kd == 1]
            q[b, h, kd == 1] = HEAD_DIM * kk[t[kd == 1]]
            ref[b, h, kd == 1] = v64[t[kd == 1]]
            if rl:
                r = (g // 3 if family == "mixed" else g) % len(rl)
                run_of[b, h, kd == 2] = r[kd == 2]
                q[b, h, kd == 2] = HEAD_DIM * kk[np.array([a for a, _ in rl])[r[kd == 2]]]
                ref[b, h, kd == 2] = np.array(run_ref)[r[kd == 2]]
            q[b, h, kd == 3] = HEAD_DIM * kk[np.array(tg)[g[kd == 3] % len(tg)]]   # padding rows would score high
            ref[b, h, kd == 3] = np.nan
    assert is_f16(q) and is_f16(k) and is_f16(v)
    return out


def round_out(x, out16):
    return f16(x) if out16 else np.asarray(x, np.float32)


def out_rounding(mag, out16):
    """Half an ulp of the output type at magnitude mag (fp32 output: the product's own rounding is in the ulp terms)."""
    if not out16:
        return np.zeros_like(mag)
    return np.maximum(U16 * mag, SUB16)


def exact_bound(ref, kind, n_splits, out16):
    """Elementwise bound of the exact families ([.., nq, 64] like ref): 0 on selector rows (compare bits), see the
    module docstring for census and two-level rows. NaN rows (past a query count) are compared as NaN."""
    mag = np.abs(ref)
    b = (6 + n_splits) * U * mag
    b = b + out_rounding(mag + b, out16)
    if n_splits > 1 and out16:
        b = b + U16 * mag + SUB16
    b[np.broadcast_to((kind == b"s")[..., None], b.shape)] = 0.0
    return b


def check_exact(got, case, n_splits, out16):
    """got [batch, heads, nq, 64] against an exact case -> worst error / bound over census and two-level rows (0 if
    none); asserts selector rows bit for bit, padded rows NaN, the bound elsewhere."""
    ref, kind = case["ref"], case["kind"]
    got = np.asarray(got)
    pad = kind == b"p"
    assert np.isnan(got[pad]).all(), "a row past its query count is not NaN"
    assert not np.isnan(got[~pad]).any(), "NaN in a real row (a poisoned key was read, or a row was not written)"
    sel = kind == b"s"
    want = round_out(ref[sel], out16).astype(got.dtype)
    same = got[sel].view(np.uint16 if got.dtype == np.float16 else np.uint32) == \
        want.view(np.uint16 if got.dtype == np.float16 else np.uint32)
    if not same.all():
        bad = np.argwhere(~same.all(-1))[0]
        idx = np.argwhere(sel)[bad[0]]
        raise AssertionError(f"selector row {tuple(idx)} (target key {case['target'][tuple(idx)]}) is not V[target]: "
                             f"{int((~same).sum())} elements differ")
    rest = ~sel & ~pad
    if not rest.any():
        return 0.0
    if out16:   # the census' constant column: n * fp32(1 / n) is within an fp32 ulp of 1, which fp16 rounds to 1
        assert (got[rest][:, HEAD_DIM - 1] == 1).all(), "the constant column of a census or two-level row is not exactly 1"
    bound = exact_bound(ref, kind, n_splits, out16)
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):   # (a bound of 0: a reference of 0 under fp32 output)
        ratio = np.where(err[rest] == 0, 0.0, err[rest] / bound[rest])
    worst = float(ratio.max())
    if not worst <= 1.0:
        at = np.argwhere(rest)[int(np.argmax(ratio.max(-1)))]
        raise AssertionError(f"row {tuple(at)} kind {kind[tuple(at)]}: error / bound {worst:.3g} "
                             f"(max error {float(err[rest].max()):.3e})")
    return worst


# ---- the graded families --------------------------------------------------------------------------------------------
GRADED = ("gauss1", "gauss3", "lazy7", "lazy8p")


def lazy_grades():
    """The sixteenths g in (0, 4.5] whose weight 2^(q~ g), q~ = fp16(8 kScaleLog2), rounds UP to fp16 by 0.55 to 0.95
    of half an ulp: a row sum taken from the unrounded weights then misses the sum of what P V used by about 2^-12
    of it, with one sign."""
    qt = float(f16(np.float32(8.0) * np.float32(SCALE_LOG2)))
    g = np.arange(1, 73) / 16.0
    w = 2.0 ** (qt * g)
    eps = (f16(w).astype(np.float64) - w) / w
    return g[(eps > 0.55 * U16) & (eps < 0.95 * U16)]


def graded_case(name, nq, nkv, seed, batch=1, heads=4):
    """q, k, v [batch, heads, n, 64] float32, fp16-exact. lazy7: only dim 0 of q is set (8.0, so q~ = 1.4423828) and
    k[j][0] = grade(tile of j), 0 in tile 0 and then rising through lazy_grades() to at most 4.5: scores 0 .. 6.49 log2
    units whatever the other dims of K hold, exact in fp32, a row maximum that rises tile by tile by less than 8 in
    all, P up to 2^6.49 and no rescale. V =
    1 + 2^-10 i, i in -4 .. 4: the outputs are near 1 and what a weight's error can do to them is small, so a row sum
    that does not match its P V shows. lazy8p: grades up to 1, but 5.75 in the last
    tile but one: 8.29 log2 units over the stale maximum 0."""
    from lightglue_amd import synth

    if name in ("gauss1", "gauss3"):
        q, k, v = synth.qkv(seed, nq, nkv, q_std=1.0 if name == "gauss1" else 3.0, batch=batch, heads=heads)
        return f16(q), f16(k), f16(v)
    nt = cdiv(nkv, TILE)
    q = np.zeros((batch, heads, nq, HEAD_DIM), np.float32)
    q[..., 0] = 8.0
    k = f16(synth.normal(seed * 5 + 1, (batch, heads, nkv, HEAD_DIM)))
    tile = np.arange(nkv) // TILE
    good = lazy_grades()
    # tile 0 holds grade 0 only (its maximum, the stale one, is 0); later tiles climb through the biased grades
    pick = (tile - 1) * (len(good) - 1) // max(1, nt - 2) - (np.arange(nkv) % 2)
    grade = np.where(tile == 0, 0.0, good[np.clip(pick, 0, len(good) - 1)])
    if name == "lazy8p":
        grade = np.minimum(grade, 1.0)
        grade[tile == max(1, nt - 2)] = 5.75
    k[..., 0] = grade.astype(np.float32)
    i = (synth.uniform24(seed * 5 + 2, batch * heads * nkv * HEAD_DIM) * 9).astype(np.int64) - 4
    v = (1.0 + i.reshape(batch, heads, nkv, HEAD_DIM) * 2.0 ** -10).astype(np.float32)
    assert is_f16(q) and is_f16(k) and is_f16(v)
    return q, k, v


def scores64(q, k):
    """The exact scores in log2 units, float64: (q . k) log2(e) / 8."""
    return (q.astype(np.float64) @ np.swapaxes(k.astype(np.float64), -1, -2)) * (math.log2(math.e) / 8)


def softmax64(q, k, v):
    """softmax(Q K^T / 8) V in float64 -> (o, p)."""
    s = scores64(q, k)
    p = np.exp2(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return p @ v.astype(np.float64), p


def graded_terms(q, k, v):
    """What graded_bound needs of the operands, whatever the plan and the output type (the costly part: compute once
    per case): o, sum_j p_j |v_j|, T1 split into its score part and sum_j p_j |v_j - o| (the part that R u16 + 2 E
    multiplies), sum_j |v_j - o|, sum_j 2^(s_j - smax), max eps without R, p."""
    q64, k64, v64 = (x.astype(np.float64) for x in (q, k, v))
    s = scores64(q, k)
    smax = s.max(-1, keepdims=True)
    p = np.exp2(s - smax)
    w = p.sum(-1, keepdims=True)
    p = p / w
    o = p @ v64
    a_j = (np.abs(q64) @ np.swapaxes(np.abs(k64), -1, -2)) * SCALE_LOG2
    ds = U16 * a_j + 80 * U * a_j + 2.0 ** -21 * (np.abs(s).max(-1, keepdims=True) + RESCALE_THR)
    eps0 = np.expm1(math.log(2.0) * ds)
    pe = p * eps0
    t1s, t1p, dev1 = np.empty_like(o), np.empty_like(o), np.empty_like(o)
    for d in range(HEAD_DIM):   # (without the [.., nq, nkv, 64] array)
        dev = np.abs(v64[..., None, :, d] - o[..., :, None, d])
        t1s[..., d] = (pe * dev).sum(-1)
        t1p[..., d] = (p * dev).sum(-1)
        dev1[..., d] = dev.sum(-1)
    return dict(o=o, pv=p @ np.abs(v64), t1s=t1s, t1p=t1p, dev1=dev1, w=w, eps0=eps0.max(-1, keepdims=True), p=p, v=v64,
                n=s.shape[-1])


def graded_bound(q, k, v, out16, ranges=None, p_roundings=1, floor_units=0.0, terms=None):
    """(ref, bound) [.., nq, 64], float64: the module docstring's bound, term by term. ranges: the (a, b) of each split
    (None or one entry: no partials). p_roundings: R. floor_units: F. terms: graded_terms(q, k, v), if at hand."""
    t = terms if terms is not None else graded_terms(q, k, v)
    o, n = t["o"], t["n"]
    c = p_roundings * U16 + 2 * E_HW
    w_floor = t["w"] * 2.0 ** -floor_units
    denom = 1.0 - (t["eps0"] + c) - SUB16 * n / w_floor
    assert (denom > 0.5).all()
    b = (t["t1s"] + c * t["t1p"] + SUB16 * t["dev1"] / w_floor) / denom
    b = b + (n + 32) * U * (t["pv"] + np.abs(o))
    b = b + (2 * E_HW + U) * np.abs(o)
    if ranges is not None and len(ranges) > 1:
        b = b + (len(ranges) + 4) * U * np.abs(o)
        if out16:
            for a, e in ranges:
                b = b + U16 * np.abs(t["p"][..., a:e] @ t["v"][..., a:e, :])
            b = b + SUB16
    b = b + out_rounding(np.abs(o) + b, out16)
    return o, b


def check_graded(got, ref, bound):
    """-> worst error / bound; asserts it is at most 1 on every element."""
    got = np.asarray(got).astype(np.float64)
    assert np.isfinite(got).all(), "NaN or Inf in the output"
    ratio = np.abs(got - ref) / bound
    worst = float(ratio.max())
    if not worst <= 1.0:
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"element {at}: |got - ref| = {abs(got[at] - ref[at]):.3e} > bound {bound[at]:.3e} "
                             f"(ratio {worst:.3g})")
    return worst


# ---- the restatement ------------------------------------------------------------------------------------------------
MUTANTS = ("drop_last", "drop_tile_first", "double_key", "swap_v_seam", "kv_shift", "zero_row_past_end", "count_minus",
           "count_plus", "equal_weights", "no_rescale", "rowsum_fp32", "unrounded_tile")


def restate(q, k, v, layout, n=None, out16=True, block_rows=32, zero_first=False, mutant=None, at=None):
    """The kernels' arithmetic in NumPy fp32 for one (batch, head): q [nq, 64], k / v [nkv, 64] fp16-exact float32,
    layout as plan_layout gives it for n keys (n: the item's count, default all rows of k). 64-key tiles, the running
    maximum of a wave's slice set by its first tile and then moved only when a row of the block of `block_rows` rows
    exceeds it by more than 8 at a rescale decision (zero_first: the streaming kernel's start from m = 0 while all
    tile-0 maxima lie within +-8), P rounded to fp16, the row sum from that fp16 P, waves merged in fp32, split partials
    rounded to the output type and merged by split_weight.
    mutant (at: the key or tile it applies to; a default is chosen from the layout):
      drop_last / count_minus  the last key is not visited        drop_tile_first  key 64 t is not visited
      double_key         key `at` is visited twice                swap_v_seam  V rows 63 and 64 (at - 1, at) exchanged
      kv_shift           K row j meets V row j + 1 in the tile that starts at `at`
      zero_row_past_end / count_plus  row n is visited as well: zeros (score 0), or what the buffers hold there
      equal_weights      split partials merged with weight 1 each   no_rescale  the maximum moves, O and l are not rescaled
      rowsum_fp32        l from the unrounded P                     unrounded_tile  P of tile `at` is not rounded
    """
    f32 = np.float32
    nkv = k.shape[0]
    n = nkv if n is None else n
    nq = q.shape[0]
    qs = f16(q.astype(f32) * f32(SCALE_LOG2))
    kx, vx = k, v
    if mutant in ("zero_row_past_end", "count_plus"):
        if mutant == "zero_row_past_end" or n >= nkv:
            kx = np.concatenate([k[:n], np.zeros((1, HEAD_DIM), f32)])
            vx = np.concatenate([v[:n], np.zeros((1, HEAD_DIM), f32)])
    if mutant == "swap_v_seam":
        at = TILE if at is None else at
        vx = v.copy()
        vx[[at - 1, at]] = vx[[at, at - 1]]
    s_all = (qs @ kx.T).astype(f32)
    blocks = [slice(a, min(a + block_rows, nq)) for a in range(0, nq, block_rows)]
    last_tile = max(t for waves in layout for w in waves for p in w for t in p)

    def keys_of(a, b):
        idx = np.arange(a, b)
        if mutant in ("drop_last", "count_minus") and b == n:
            idx = idx[:-1]
        if mutant == "drop_tile_first" and a == (TILE * ((n - 1) // TILE) if at is None else at) and n > 1:
            idx = idx[1:]
        if mutant == "double_key" and a <= (n // 2 if at is None else at) < b:
            idx = np.sort(np.r_[idx, n // 2 if at is None else at])
        if mutant in ("zero_row_past_end", "count_plus") and (a, b) == last_tile:
            idx = np.r_[idx, n]
        return idx

    parts = []
    for waves in layout:
        ws = []
        for w in waves:
            m = np.zeros(nq, f32)
            l = np.zeros(nq, f32)
            o = np.zeros((nq, HEAD_DIM), f32)
            first = True
            for p in w:
                if first and len(p) > 1:    # the single-pass kernels: tile 0 sets the maximum, the rest of the pass decides once
                    groups = [p[:1], p[1:]]
                else:
                    groups = [p]
                for grp in groups:
                    idx = [keys_of(a, b) for a, b in grp]
                    cat = np.concatenate(idx)
                    if len(cat) == 0:
                        continue
                    sc = s_all[:, cat]
                    mx = sc.max(1)
                    if first:
                        first = False
                        if zero_first:
                            for bl in blocks:
                                if (np.abs(mx[bl]) > RESCALE_THR).any():
                                    m[bl] = mx[bl]
                        else:
                            m = mx.copy()
                    else:
                        ex = mx - m
                        for bl in blocks:
                            if (ex[bl] > RESCALE_THR).any():
                                d = np.maximum(ex[bl], f32(0))
                                alpha = np.exp2(-d).astype(f32)
                                if mutant != "no_rescale":
                                    o[bl] *= alpha[:, None]
                                    l[bl] *= alpha
                                m[bl] = m[bl] + d
                    for (a, b), ix in zip(grp, idx):
                        if len(ix) == 0:
                            continue
                        with np.errstate(over="ignore"):
                            e = np.exp2(s_all[:, ix] - m[:, None]).astype(f32)
                        ph = e if (mutant == "unrounded_tile" and a == (0 if at is None else at)) else f16(e)
                        vt = vx[ix]
                        if mutant == "kv_shift" and a == (0 if at is None else at):
                            vt = vx[np.minimum(ix + 1, len(vx) - 1)]
                        l += (e if mutant == "rowsum_fp32" else ph).sum(1, dtype=f32)
                        o += (ph @ vt).astype(f32)
            ws.append((np.where(l > 0, m, -np.inf).astype(f32), l, o))
        M = np.max([x[0] for x in ws], 0)
        L = np.zeros(nq, f32)
        acc = np.zeros((nq, HEAD_DIM), f32)
        for mw, lw, ow in ws:
            with np.errstate(invalid="ignore"):
                wt = np.where(np.isneginf(mw), f32(0), np.exp2(mw - M)).astype(f32)
            L += wt * lw
            acc += wt[:, None] * ow
        parts.append((M, L, acc))
    with np.errstate(divide="ignore", invalid="ignore"):
        if len(parts) == 1:
            M, L, acc = parts[0]
            return round_out(acc * (f32(1) / L)[:, None], out16)
        Mt = np.max([x[0] for x in parts], 0)
        Lt = np.zeros(nq, f32)
        acc_t = np.zeros((nq, HEAD_DIM), f32)
        for M, L, acc in parts:
            inv = np.where(L > 0, f32(1) / L, f32(0)).astype(f32)
            part = round_out(acc * inv[:, None], out16)
            wt = np.ones(nq, f32) if mutant == "equal_weights" else \
                np.where(np.isneginf(M), f32(0), np.exp2(M - Mt) * L).astype(f32)
            Lt += wt
            acc_t += wt[:, None] * part
        return round_out(acc_t * (f32(1) / Lt)[:, None], out16)
