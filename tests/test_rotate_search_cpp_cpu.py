"""The host C++ of the unknown-angle row, as stand-alone programs (each has its own main; nothing is loaded into Python):
csrc/angle_share.hpp -- the share-groups of the shared angle search, the unions of their members' candidates and who wants what
-- against a Python restatement on hand-made slot lists, and wm::rotate_search_attack (include/ssw_rotate_search.hpp) over a
contract stub.  Both plain and under ASan/UBSan."""
import subprocess

import numpy as np
import pytest

from test_angle_cpu import build_exe

SLOTS, SHARE_MAX, NONE, SKIP = 60, 16, 255, -(1 << 31)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def share_groups_ref(keys):
    """[[suspects]]: suspects of one key in the order they come, in chunks of 16; groups in the order of their first member"""
    groups, open_group = [], {}
    for i, k in enumerate(keys):
        if k not in open_group or len(groups[open_group[k]]) == SHARE_MAX:
            open_group[k] = len(groups)
            groups.append([])
        groups[open_group[k]].append(i)
    return groups


def share_cands_ref(slots, groups):
    """per group [(angle, mask, [slot of member m or 255])]: the union of the members' angles, ascending"""
    out = []
    for members in groups:
        union = sorted({a for s in members for a in slots[s] if a != SKIP})
        cands = []
        for a in union:
            where = [slots[s].index(a) if a in slots[s] else NONE for s in members] + [NONE] * (SHARE_MAX - len(members))
            cands.append((a, sum(1 << m for m, t in enumerate(where) if t != NONE), where))
        out.append(cands)
    return out


def slot_list(rungs, lo=-320, hi=320):
    """A slot list as angle_keep_kernel leaves it: 15 angles around each of up to 4 kept rungs (angles n = 8 j), those outside
    lo .. hi or owned by an earlier rung skipped"""
    out = []
    for k in range(4):
        for e in range(15):
            a = SKIP
            if k < len(rungs):
                a = 8 * rungs[k] + e - 7
                if not lo <= a <= hi or any(abs(a - 8 * r) <= 7 for r in rungs[:k]):
                    a = SKIP
            out.append(a)
    return out


def cases():
    rng = np.random.default_rng(5)
    near = lambda j: [int(v) for v in j + rng.permutation(4) - 1]
    yield "one suspect", [0], [slot_list([5, 4, 6, 3])]
    yield "identical lists", [7] * 5, [slot_list([5, 4, 6, 3])] * 5
    yield "disjoint lists", [1, 1, 1], [slot_list([-30, -31, -29, -28]), slot_list([0, 1, 2, 3]), slot_list([30, 33, 36, 39])]
    yield "all-skip lists beside a full one", [2, 2, 2], [[SKIP] * SLOTS, slot_list([1, 2]), [SKIP] * SLOTS]
    yield "every list all-skip", [3, 3], [[SKIP] * SLOTS] * 2
    yield "exactly 16 members", [4] * 16, [slot_list(near(10)) for _ in range(16)]
    yield "17 members: the chunk boundary", [4] * 17, [slot_list(near(-8)) for _ in range(17)]
    yield "two keys interleaved, the range's edge", [0, 1] * 10, [slot_list(near(39 if i % 2 else -39)) for i in range(20)]
    yield "a list with fewer than 4 rungs", [9, 9], [slot_list([0]), slot_list([1, 0])]
    yield "33 members of one key beside 2 of another", [5] * 20 + [6] + [5] * 13 + [6], [slot_list(near(i % 7)) for i in range(35)]


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def share_exe(request, tmp_path_factory):
    return build_exe(tmp_path_factory.mktemp("angle_share"), "angle_share_test", ["angle_share_test.cpp"], request.param)


@pytest.mark.parametrize("name,keys,slots", list(cases()), ids=[c[0] for c in cases()])
def test_share_groups_unions_and_masks(share_exe, tmp_path, name, keys, slots):
    assert all(len(s) == SLOTS for s in slots) and len(keys) == len(slots)
    path = tmp_path / "case.txt"
    path.write_text("\n".join([str(len(keys)), " ".join(map(str, keys))] + [" ".join(map(str, s)) for s in slots]) + "\n")
    out = subprocess.run([share_exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    lines = [line.split() for line in out.stdout.splitlines()]
    got_groups = [[int(v) for v in line[1:]] for line in lines if line[0] == "G"]
    got_cands = [[int(v) for v in line[1:]] for line in lines if line[0] == "C"]
    groups = share_groups_ref(keys)
    cands = share_cands_ref(slots, groups)
    first = np.cumsum([0] + [len(c) for c in cands])
    assert got_groups == [[len(g), int(first[i]), len(cands[i])] + g for i, g in enumerate(groups)]
    assert got_cands == [[a, mask] + where for c in cands for a, mask, where in c]
    # what the kernel relies on: at most 16 members; every (member, angle of its list) is wanted once, at its own slot
    assert all(1 <= len(g) <= SHARE_MAX for g in groups) and sorted(s for g in groups for s in g) == list(range(len(keys)))
    for g, c in zip(groups, cands):
        for m, s in enumerate(g):
            mine = {a: t for a, mask, where in c for t in [where[m]] if mask >> m & 1}
            assert mine == {a: t for t, a in enumerate(slots[s]) if a != SKIP}
        assert all(mask and not mask >> len(g) for _, mask, _ in c)


def test_the_cases_cover_what_they_name():
    by_name = {name: (keys, slots) for name, keys, slots in cases()}
    assert [len(g) for g in share_groups_ref(by_name["exactly 16 members"][0])] == [16]
    assert [len(g) for g in share_groups_ref(by_name["17 members: the chunk boundary"][0])] == [16, 1]
    assert [len(g) for g in share_groups_ref(by_name["33 members of one key beside 2 of another"][0])] == [16, 16, 2, 1]
    keys, slots = by_name["disjoint lists"]
    assert all(bin(mask).count("1") == 1 for _, mask, _ in share_cands_ref(slots, share_groups_ref(keys))[0])
    keys, slots = by_name["identical lists"]
    assert all(mask == 31 for _, mask, _ in share_cands_ref(slots, share_groups_ref(keys))[0])
    keys, slots = by_name["every list all-skip"]
    assert share_cands_ref(slots, share_groups_ref(keys)) == [[]]
    keys, slots = by_name["17 members: the chunk boundary"]
    assert len({tuple(s) for s in slots}) > 1                          # members of one group with different lists


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_cpp_wrapper_against_a_stub(tmp_path, sanitize):
    """wm::rotate_search_attack over a stub of the C function: argument order, vector sizes, the optional outputs, a thrown
    status with nothing left alive"""
    exe = build_exe(tmp_path, "rotate_search_wrappers_test",
                    ["rotate_search_wrappers_test.cpp", "rotate_search_stub.cpp", "angle_stub.cpp", "ssw_stub.cpp"], sanitize)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert out.stdout.splitlines()[-1] == "rotate search wrappers: ok"
