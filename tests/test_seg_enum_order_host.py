"""The ORDER in which the enumeration launch hands out its candidates (pngloss_amd/csrc/pl_seg_launch.h: seg_dispatch_enum), on the CPU through the recording
stubs of tests/c/seg_launch_host.cpp: the workgroups of a launch start in the order of their index, a CU's oldest waves issue first, and the launch ends with
its last workgroup -- so the candidate with the longest workgroups (paeth) comes first and the shortest of those that look at the left pixel (sub) last.
tests/test_seg_launch_host.py says that every piece of work is visited exactly once whatever the order; this file pins the order, which is worth 0.9 us a
launch on the headline row (profiles/r11_enum_tail_placement.txt)."""
import pytest

from tests import test_seg_launch_host as TL

NONE, SUB, UP, AVG, PAETH = range(5)


def candidates_in_dispatch_order(shape, W):
    k = TL.consts()
    visits = TL.c_visits(shape, 0, W, 4, 0, 0, 0, [0] * k.NFILT)
    launch = [v[0] for v in visits if v[1] == TL.ENUM][0]
    seen = []
    for v in visits:                                   # (launch, body, template arguments x 2, par, f, segment, channel group): in the order of the workgroups' index
        if v[0] == launch and v[1] == TL.ENUM and (not seen or seen[-1] != v[5]):
            seen.append(v[5])
    bodies = [v[1] for v in visits if v[0] == launch]
    return seen, bodies


@pytest.mark.parametrize("nt", [512, 1024])
@pytest.mark.parametrize("nseg", [1, 5, 128])
def test_longest_candidate_first_with_none_and_up_from_their_tables(nt, nseg):
    k = TL.consts()
    seen, bodies = candidates_in_dispatch_order(TL.make_shape(nseg, nt, k.TPARTS, 1, True, False, False), nseg * k.L)
    assert seen == [PAETH, AVG, SUB]
    # ... and all of them in front of the short workgroups of none / up and the walkers of an epoch's first segment
    last_enum = max(i for i, b in enumerate(bodies) if b == TL.ENUM)
    assert all(b == TL.ENUM for b in bodies[:last_enum + 1]) and set(bodies[last_enum + 1:]) == {TL.ENUM_SMALL, TL.FIRST}


@pytest.mark.parametrize("nt", [512, 1024])
def test_longest_candidate_first_with_all_five_enumerated(nt):
    k = TL.consts()
    seen, _ = candidates_in_dispatch_order(TL.make_shape(7, nt, k.TPARTS, 1, False, False, False), 7 * k.L - 3)
    assert seen == [PAETH, AVG, UP, SUB, NONE]
