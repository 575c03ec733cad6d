"""The preconditions the GPU tests of the bundle adjustment rest on (test_gpu_bundle.py), from the float64 reference alone:
every scene's reference converges, every window has the observations the contract asks for, no residual lies near a
decision, and the dirty rows are dropped. No GPU."""
import numpy as np
import pytest

import bundle_scenes as bs
from lightglue_amd import bundle_adjust_reference, bundle_fixed_set
from lightglue_amd.geometry_contract import _bundle_residuals


@pytest.mark.parametrize("views,k", bs.CASES)
def test_reference_converges_on_a_well_posed_window(views, k):
    w, ref = bs.window(bs.scene(views, k)), bs.reference(views, k)
    mask, usable, res = bundle_fixed_set(*w)
    assert usable and int(ref.kept) == 1 and int(ref.num_obs) == int(mask.sum())
    assert (mask.sum(0)[mask.any(0)] >= 2).all() and (mask[1:].sum(1) >= 4).all()
    assert 2 * int(mask.sum()) > 6 * views - 7 + 3 * int(mask.any(0).sum())  # more residuals than parameters
    # the only decisions are a finite residual at a positive depth: under the entering state every seen observation is
    # far inside both (a depth above 1 where the decision is at 0; a residual of a few hundred px at most)
    seen = w[1].numpy() != 0
    r0 = np.concatenate([np.eye(3)[None], w[4].double().numpy()[1:]])
    t0 = np.concatenate([np.zeros((1, 3)), w[5].double().numpy()[1:]])
    _, depth = _bundle_residuals(r0, t0, w[6].double().numpy(), w[0].double().numpy(), w[3].double().numpy())
    assert np.array_equal(mask.any(0)[None, :] & seen, mask) and np.abs(res[mask]).max() < 1e3 and depth[seen].min() > 1.0
    assert float(ref.cost[1]) < 0.05 * float(ref.cost[0])
    # the gradient at the floor: a second run from the minimiser moves nothing
    again = bundle_adjust_reference(w[0], w[1], w[2], w[3], ref.R.float(), ref.t.float(), ref.points.float())
    assert abs(float(again.cost[1] if int(again.kept) else again.cost[0]) - float(ref.cost[1])) <= 1e-5 * float(ref.cost[1])


def test_dirty_rows_are_dropped():
    wins, rows = bs.dirty_windows()
    clean, _, _ = bundle_fixed_set(*wins[2])
    dirty, usable, _ = bundle_fixed_set(*wins[4])
    assert usable and not dirty[1, rows[0]] and dirty[0, rows[0]] and not dirty[:, rows[1]].any() and not dirty[:, rows[2]].any()
    assert int(dirty.sum()) == int(clean.sum()) - 1 - 3 - 3
    for i in (0, 1, 3, 5):
        assert not bundle_fixed_set(*wins[i])[1] and int(bundle_adjust_reference(*wins[i]).kept) == 0, i


def test_float64_chain_with_bundle_adjustment_beats_the_chain_without():
    """View 2 against the truth on the three-view scene: 2.313e-2 deg and 9.898e-4 without, 1.802e-2 deg and 7.693e-4 with
    (ratios 0.779 and 0.777): the source of test_gpu_bundle.CHAIN_RATIO."""
    without, with_ba, w, ref = bs.chain_reference()
    print(f"view 2 without {without}, with {with_ba}")
    mask, usable, _ = bundle_fixed_set(*w)
    assert usable and int(ref.kept) == 1 and mask[2].sum() >= 50
    assert with_ba[0] < 0.8 * without[0] and with_ba[1] < 0.8 * without[1]
