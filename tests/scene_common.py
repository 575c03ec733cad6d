"""What geometry_scenes.py, homography_scenes.py, essential_scenes.py and polish_scenes.py build alike: a scene through
the matcher's layout, batches of such pairs, and the scoring inputs' planted rows. A plain module: no fixtures, no
GPU."""
import torch


def shuffled_pair(k0, k1, generator_seed):
    """Keypoints k0, k1 [k, 2] through the matcher's layout: (matches [k, 2] int32, kpts0 [k, 2], kpts1 [k, 2]) with
    the keypoints of each image in a shuffled order of their own; correspondence j is the scene's row j."""
    k = len(k0)
    gen = torch.Generator().manual_seed(generator_seed)
    p0, p1 = torch.randperm(k, generator=gen), torch.randperm(k, generator=gen)
    kp0, kp1 = torch.empty_like(k0), torch.empty_like(k1)
    kp0[p0], kp1[p1] = k0, k1
    return torch.stack([p0, p1], 1).int(), kp0, kp1


def batch_of(pair_fn, specs, kmax):
    """specs: (scene, count) per pair, pair_fn(scene) -> shuffled_pair's three -> (matches [P, kmax, 2] with -1 past
    the count, counts [P], kpts0, kpts1 [P, max k, 2] zero-padded)."""
    pairs = [pair_fn(scene) for scene, _ in specs]
    kk = max(len(a) for _, a, _ in pairs)
    m = torch.full((len(specs), kmax, 2), -1, dtype=torch.int32)
    kp0, kp1 = torch.zeros((len(specs), kk, 2)), torch.zeros((len(specs), kk, 2))
    for p, ((_, count), (mm, a, b)) in enumerate(zip(specs, pairs)):
        k = len(a)
        m[p, :count], kp0[p, :k], kp1[p, :k] = mm[:count], a, b
    return m, torch.tensor([c for _, c in specs], dtype=torch.int32), kp0, kp1


def plant_dirty_rows(m, kp0, kp1, k):
    """One pair's matches m and keypoint tables of k + 8 rows: match indices out of range on both sides (rows 5, 6)
    and NaN and Inf keypoints (those of rows 10, 11, 12)."""
    m[5], m[6] = torch.tensor([-7, k + 500]).int(), torch.tensor([k + 8, -1]).int()
    kp0[int(m[10, 0])] = float("nan")
    kp1[int(m[11, 1]), 0] = float("inf")
    kp0[int(m[12, 0]), 1] = float("-inf")


def score_inputs(k0, k1, cands, counts, error, threshold, margin, plant=None):
    """The scoring kernels' inputs on a scene of k rows (k0, k1 [k, 2]; cands [C, 3, 3] fp32 numpy; error(c, x0, x1):
    float64 squared pixels): (matches [P, k, 2], counts, kpts0, kpts1 [P, k + 8, 2], candidates [P, C, 9] fp32, want
    [P, C] int32), each pair its own shift of the rows. From 63 rows on a pair gets plant_dirty_rows, then
    plant(p, m, kp0): what else the caller moves. Rows whose error under a candidate lies within margin of the
    threshold are moved until none does."""
    from lightglue_amd.geometry import gather_correspondences

    k, pr = len(k0), len(counts)
    m = torch.full((pr, k, 2), -1, dtype=torch.int32)
    kp0, kp1 = torch.zeros((pr, k + 8, 2)), torch.zeros((pr, k + 8, 2))
    want = torch.zeros((pr, len(cands)), dtype=torch.int32)
    for p, count in enumerate(counts):
        idx = (torch.arange(k) + 97 * p) % k
        kp0[p, :k], kp1[p, :k] = k0, k1
        kp0[p, k:], kp1[p, k:] = k0[:8], k1[-8:]          # rows that only a clamped index reaches
        m[p, :count] = torch.stack([idx, idx], 1)[:count].int()
        if count >= 63:
            plant_dirty_rows(m[p], kp0[p], kp1[p], k)
            if plant is not None:
                plant(p, m, kp0)
        for _ in range(50):
            x0, x1 = gather_correspondences(m[p], count, kp0[p], kp1[p])
            err = torch.stack([error(c, x0, x1).sqrt() for c in cands])
            near = ((err - threshold).abs() <= margin).any(0)
            if not bool(near.any()):
                break
            for j in torch.nonzero(near)[:, 0].tolist():
                kp1[p, int(m[p, j, 1].clamp(0, k + 7))] += torch.tensor([7.3, -5.1])
        assert not bool(near.any()), "score_inputs: rows within the margin of the threshold remain"
        want[p] = (err <= threshold).sum(1).int()  # (NaN and Inf compare false)
    return m, torch.tensor(counts, dtype=torch.int32), kp0, kp1, torch.from_numpy(cands).reshape(1, -1, 9).repeat(pr, 1, 1), want
