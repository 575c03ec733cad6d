"""What the GPU tests share: bitwise comparison, the seeded matcher, the warm-up and capture of a run on a side
stream, and guarded device buffers for calls made through raw pointers. A plain module: no fixtures."""
import torch

GUARD_BYTES = 4096      # on both sides of a guarded output, and behind a guarded input
SENTINEL_BYTE = 0xA5    # the guards of an output (0xA5A5 is a finite fp16, 0xA5A5A5A5 a finite fp32)


class GuardedOut:
    """An output of `shape` / `dtype` as a view inside a larger allocation: GUARD_BYTES (+ `shift`, for a pointer that
    is 8-B but not 16-B aligned) of SENTINEL_BYTE before it and GUARD_BYTES after it, the region itself NaN. ptr: its
    address (an empty output has one too). check(): the guards unchanged and no NaN left inside -> the CPU copy."""

    def __init__(self, shape, dtype, dev, shift=0, fill=None):
        self.numel = 1
        for d in shape:
            self.numel *= int(d)
        es = torch.empty((), dtype=dtype).element_size()
        assert shift % es == 0
        self.lo = GUARD_BYTES + shift
        self.hi = self.lo + self.numel * es
        self.buf = torch.full((self.hi + GUARD_BYTES,), SENTINEL_BYTE, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.hi].view(dtype).view(*shape)
        if fill is None:
            self.view.fill_(float("nan"))
        else:  # (an in-place call: the region starts as the input)
            self.view.copy_(fill)
        self.ptr = self.buf.data_ptr() + self.lo

    def check(self, what=""):
        assert bool((self.buf[:self.lo] == SENTINEL_BYTE).all()), f"{what}: wrote before the output"
        assert bool((self.buf[self.hi:] == SENTINEL_BYTE).all()), f"{what}: wrote past the output"
        out = self.view.cpu()
        assert not bool(torch.isnan(out).any()), f"{what}: {int(torch.isnan(out).sum())} elements not written (or NaN)"
        return out


class GuardedIn:
    """A row-indexed input on the device with NaN all round it: 256 B (+ `shift`) before, GUARD_BYTES after, so a
    read past its last row that reaches a result shows there. ptr: the address of its first element."""

    def __init__(self, t, dev, shift=0):
        es = t.element_size()
        assert shift % es == 0 and t.dtype in (torch.float16, torch.float32)
        pre = (256 + shift) // es
        self.buf = torch.full((pre + t.numel() + GUARD_BYTES // es,), float("nan"), dtype=t.dtype, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[pre:pre + t.numel()].view(*t.shape)
        self.view.copy_(t)
        self.ptr = self.buf.data_ptr() + pre * es


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def equal_results(a, b, what):
    for name, x, y in zip(a._fields, a, b):
        assert same_bits(x, y), (what, name)


def seeded_matcher(dev, n_layers=3, seed=7):
    from lightglue_amd import matcher

    m = matcher.LightGlueMatcher(n_layers=n_layers).eval()
    m.load_state_dict(matcher.seeded_state_dict(seed, n_layers), strict=True)
    return m.to(dev, torch.float16)


def capture_on_side_stream(run, on_side=True):
    """run() once on a side stream off the capture (caches, packed weights, workspaces), then captured: (graph,
    what the captured run returned). on_side: capture on that same stream, else on torch's own capture stream."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=side if on_side else None):
        outputs = run()
    return graph, outputs
