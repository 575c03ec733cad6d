"""What the GPU tests of the image-to-matches path share: bitwise comparison, the seeded matcher, and the
warm-up and capture of a run on a side stream. A plain module: no fixtures."""
import torch


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
