"""Every kernel instance csrc/kernel_instances.h lists is launched by a program of tests/instance_programs.py: PROGRAMS - on the CPU,
from the host-only plan description (edmp_unet_plan_describe).  tests/test_gpu_instances.py runs those programs on the GPU.

An instance that is compiled, shipped and selectable through a documented switch but launched by no test is how the four-sample level
kernels and the direct-form L = 4 Conv1dBlocks went unexecuted; adding a line to kernel_instances.h without a program that runs it,
or deleting a row of PROGRAMS that was the only one to reach an instance, fails here."""
import fnmatch
import re

from tests import instance_programs as P

NAME = re.compile(r"^(wide_conv_kernel|bf3_conv_kernel)<\d+, (16|32), \d+, \d+, \d+, (true|false)>$|^level_kernel<[012], (32|64), \d+, [24], \d+>$|"
                  r"^level2_kernel<[012], (32|64), \d+, \d+, [012], (32|64), \d+, \d+, [24]>$")


def test_every_listed_name_parses():
    names = P.listed_instances()
    assert len(names) == 56 and len(set(names)) == 56, len(names)  # 30 wide + 16 bf3 + 8 level + 2 level2 today
    by_family = {f: sum(n.startswith(f + "<") for n in names) for f in ("wide_conv_kernel", "bf3_conv_kernel", "level_kernel", "level2_kernel")}
    assert by_family == {"wide_conv_kernel": 30, "bf3_conv_kernel": 16, "level_kernel": 8, "level2_kernel": 2}, by_family
    for n in names:
        assert NAME.match(n), n


def test_a_merged_pair_counts_as_one_launch():
    """EDMP_LEVEL_SB=4444 alone describes level_kernel<2, 32, 25, 4, 128> beside the level2_kernel that runs in its place (the pair's
    tile height is its own): the name of the op behind a merged pair is not a launch"""
    raw = ["level2_kernel<0, 32, 50, 8, 0, 64, 25, 32, 2>", "level_kernel<0, 64, 25, 4, 32>", "bf3_conv_kernel<0, 32, 64, 64, 4, true>",
           "level2_kernel<1, 64, 13, 256, 2, 32, 25, 128, 2>", "level_kernel<2, 32, 25, 4, 128>"]
    assert P.launched(raw) == [raw[0], raw[2], raw[3]]
    merged = P.described(("A2", {"EDMP_LEVEL_SB": "4444"}))
    assert "level2_kernel<1, 64, 13, 256, 2, 32, 25, 128, 2>" in merged and not any(n.startswith("level_kernel<") for n in merged), merged
    split = P.described(("A2", {"EDMP_LEVEL_SB": "4444", "EDMP_LEVEL_MERGE": "0"}))
    assert "level_kernel<2, 32, 25, 4, 128>" in split and not any(n.startswith("level2_kernel<") for n in split)


def test_the_programs_reach_every_listed_instance():
    """the union over PROGRAMS of what the plans launch holds every listed instance"""
    listed = P.listed_instances()
    reached = set()
    for row in P.PROGRAMS:
        reached |= set(P.described(row))
    missing = [n for n in listed if n not in reached]
    assert not missing, "listed in csrc/kernel_instances.h but launched by no program of tests/instance_programs.py: " + ", ".join(missing)


def test_every_listed_instance_belongs_to_one_row_that_launches_it():
    """the rows' `there_for` patterns split the list: no instance unclaimed (a new line of kernel_instances.h, a deleted row), none claimed
    twice, no pattern that matches nothing, and a row's plan launches what the row claims (what tests/test_gpu_instances.py asserts of
    the bound program)"""
    listed = P.listed_instances()
    owner = {}
    for row in P.PROGRAMS:
        names = set(P.described(row))
        for pat in row.there_for:
            assert any(fnmatch.fnmatchcase(n, pat) for n in listed), (P.program_id(row), pat)
        for n in P.there_for(row, listed):
            assert n not in owner, (n, owner[n], P.program_id(row))
            owner[n] = P.program_id(row)
            assert n in names, f"{P.program_id(row)} claims {n} and does not launch it"
    unclaimed = [n for n in listed if n not in owner]
    assert not unclaimed, "no row of tests/instance_programs.py: PROGRAMS answers for " + ", ".join(unclaimed)


def test_describing_a_program_leaves_the_environment_alone():
    import os

    before = dict(os.environ)
    P.described(P.PROGRAMS[0])
    assert dict(os.environ) == before
