"""GPU: the search partition (psg_partition.hip search_item: edge lanes that
search the whole push, the lanes between bracketed by their answers), forced
with PSG_PART_SEARCH -- every cut is checked through the merge: sums bit for
bit and matched counts against the oracle (a wrong cut leaves keys
unmatched), and the same through PSG_PART_STREAM.  Waves whose last group
holds 1, 2 or 64 boundaries; pushes that are empty, hold one key, lie below
or above D or inside one tile, grow geometrically (interpolation is wrong in
every bracket), or start at every 8-B offset of a 128-B line."""
import numpy as np
import pytest

import index_inputs as I
import oracle_py as O
from test_index_nibbles_gpu import ALL, assert_bitexact, plan_for, to_dev, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

NTILES = [1, 15, 16, 17, 63, 64, 65]  # the last wave holds 2, 16, 17, 18, 64, 1, 2 valid lanes


_cases = {}


def case(ntiles):
    if ntiles not in _cases:
        D, ps = I.partition_case(ntiles)
        _, _, _, want, wm = O.aggregate(D, *ALL, ps)
        _cases[ntiles] = (D, ps, np.array(want[0]), [int(x) for x in wm])
    return _cases[ntiles]


def arena_plan(torch, D, pushes, flags):
    """plan_for with the last 16 pushes' keys as views at offsets 0..15 keys
    into one 128-B aligned allocation."""
    from parameter_server_amd.kv_vector import MergePlan
    from parameter_server_amd._lib import PSG_F32
    starts, cur = [], 0
    for o in range(16):
        cur += (o - cur) % 16
        starts.append(cur)
        cur += pushes[-16 + o][0].size
    arena = np.zeros(cur + 16, np.uint64)
    for o, s in enumerate(starts):
        k = pushes[-16 + o][0]
        arena[s:s + k.size] = k
    dar = to_dev(torch, arena)
    assert dar.data_ptr() % 128 == 0
    dD = to_dev(torch, D)
    pk = [to_dev(torch, k) for k, _ in pushes[:-16]]
    pk += [dar[s:s + pushes[-16 + o][0].size] for o, s in enumerate(starts)]
    for o, t in enumerate(pk[-16:]):
        assert (t.data_ptr() % 128) // 8 == o
    pv = [[to_dev(torch, v) for v in vs] for _, vs in pushes]
    out = [torch.full((D.size,), float("nan"), dtype=torch.float32, device="cuda")]
    job = {"keys": dD.data_ptr(), "nslots": D.size,
           "push_keys": [t.data_ptr() for t in pk],
           "push_vals": [[t.data_ptr() for t in vs] for vs in pv],
           "push_n": [k.size for k, _ in pushes],
           "out": [o.data_ptr() for o in out]}
    return MergePlan(0, PSG_F32, 1, [job], False, flags), (dD, dar, pk, pv, out)


@pytest.mark.parametrize("mode", ["search", "stream"])
@pytest.mark.parametrize("ntiles", NTILES)
def test_cuts_through_the_merge(torch_cuda, ntiles, mode):
    from parameter_server_amd import _lib as L
    D, ps, want, wm = case(ntiles)
    flags = L.PSG_FORM_UNIFORM | (L.PSG_PART_SEARCH if mode == "search" else L.PSG_PART_STREAM)
    plan, keep = arena_plan(torch_cuda, D, ps, flags)
    for _ in range(2):
        plan.run()
        assert plan.matched().tolist() == wm
        assert_bitexact(keep[4][0].cpu().numpy(), want)
    # the inputs are what they claim: nothing of the below/above pushes matches
    assert wm[1] == 0 and wm[2] == 1 and wm[3] == 0 and wm[4] == 0 and wm[5] == 100
    assert wm[6] == ps[6][0].size
    plan.close()


@pytest.mark.parametrize("ntiles", [17, 65])
def test_unsorted_push_terminates_and_is_reported(torch_cuda, ntiles):
    from parameter_server_amd import _lib as L
    D, ps, want, wm = case(ntiles)
    bad = [(k.copy(), vs) for k, vs in ps]
    for which in (0, 6):  # the regular and the geometric push, two blocks swapped
        kb = bad[which][0]
        n = kb.size
        a = kb[n // 8: n // 8 + 40].copy()
        kb[n // 8: n // 8 + 40] = kb[n - 100: n - 60]
        kb[n - 100: n - 60] = a
    plan, keep = arena_plan(torch_cuda, D, bad, L.PSG_FORM_UNIFORM | L.PSG_PART_SEARCH)
    plan.run()
    mt = plan.matched().tolist()
    assert mt[0] < ps[0][0].size and mt[6] < ps[6][0].size
    assert [x for i, x in enumerate(mt) if i not in (0, 6)] == \
           [x for i, x in enumerate(wm) if i not in (0, 6)]
    plan.close()
