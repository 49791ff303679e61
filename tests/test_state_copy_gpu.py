"""-m gpu: the state-copy launch (k_state_copy, hip_backend.hip match_state_copies) alone, through the C-ABI: runs of flat column copies between
[len, C, 3] F32 tensors and 16-byte-aligned slices of a staging tensor, with columns of 24 bytes (8- and 16-aligned bases), 60 bytes (4-aligned
columns only), 512 bytes and 492 544 bytes (31 pieces, the last one partial). Every tensor is prefilled with its own random bit pattern and compared
whole, as uint32, with what numpy makes of the same copies: the jobs' bytes arrive and no byte outside them changes, the other columns of the same
tensors included. The same graph under backend flag 1 (generic copies) must give the same bytes.

Three kinds of copy make a run - column 1 -> column 2, column 2 -> a staging slice, a staging slice -> column 0. Within one tensor the second would
read what the first writes, which the matcher declines (see the declined runs below), so each shape holds one tensor per kind."""
import numpy as np
import pytest

from ggml_util import F32, Graph

pytestmark = pytest.mark.gpu

SHAPES = [(6, 1), (5, 3), (2, 64), (1924, 64)]   # (len, C): columns of 24, 60, 512 and 492 544 bytes
B = 3


def pad4(n):
    return (n + 3) // 4 * 4


class Case:
    """tensors with known contents, a list of copies, and numpy's version of the result"""

    def __init__(self, g, seed=5):
        self.g, self.rng = g, np.random.default_rng(seed)
        self.tensors, self.host, self.copies = [], [], []

    def tensor(self, *ne):
        n = int(np.prod(ne))
        bits = self.rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        t = self.g.input_raw(bits, F32, *ne)
        self.tensors.append(t)
        self.host.append(bits.copy())
        return len(self.tensors) - 1

    def column(self, i, ln, c, b):
        """column b of the [ln, c, B] tensor i -> (view, tensor index, first element, elements)"""
        return self.g.view_2d(self.tensors[i], ln, c, ln * 4, b * ln * c * 4), i, b * ln * c, ln * c

    def piece(self, i, ln, c, first):
        """ln x c elements of the 1-D tensor i from element `first` on, as a [ln, c] view"""
        assert first % 4 == 0                                        # a 16-byte boundary
        return self.g.view_2d(self.tensors[i], ln, c, ln * 4, first * 4), i, first, ln * c

    def copy(self, src, dst):
        self.copies.append(self.g.cpy(src[0], dst[0]))
        assert src[3] == dst[3]
        self.host[dst[1]][dst[2]:dst[2] + dst[3]] = self.host[src[1]][src[2]:src[2] + src[3]].copy()   # in graph order, as a generic plan runs them

    def run(self):
        g = self.g
        g.build(self.copies)
        g.alloc()
        g.compute()
        got = [g.get(t).view(np.uint32).reshape(-1) for t in self.tensors]
        return got, g.stats()


def three_kinds(g):
    c = Case(g)
    total = sum(pad4(ln * ch) for ln, ch in SHAPES)
    out, inp = c.tensor(total), c.tensor(total)
    off = 0
    for ln, ch in SHAPES:
        x, y, z = c.tensor(ln, ch, B), c.tensor(ln, ch, B), c.tensor(ln, ch, B)
        c.copy(c.column(x, ln, ch, 1), c.column(x, ln, ch, 2))
        c.copy(c.column(y, ln, ch, 2), c.piece(out, ln, ch, off))
        c.copy(c.piece(inp, ln, ch, off), c.column(z, ln, ch, 0))
        off += pad4(ln * ch)
    return c


def run_case(build, flags=0):
    g = Graph("hip", mem_mb=16)
    try:
        if flags:
            g.set_flags(flags)
        c = build(g)
        got, st = c.run()
        return got, [h.copy() for h in c.host], st
    finally:
        g.free()


def check(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{what}: tensor {i} of {a.size} elements: {bad.size} differ, the first at element {bad[0]}"


def test_one_launch_copies_every_job_and_nothing_else():
    got, want, st = run_case(three_kinds)
    print(f"{st.kernels_in_last_plan} launches, {st.state_copy_launches_in_last_plan} state-copy launches holding {st.state_copy_jobs_in_last_plan} jobs")
    assert st.state_copy_launches_in_last_plan == 1 and st.state_copy_jobs_in_last_plan == 3 * len(SHAPES)
    assert st.kernels_in_last_plan == 1 and st.ring_copy_launches_in_last_plan == 0
    check(got, want, "one launch")
    generic, _, st1 = run_case(three_kinds, flags=1)
    assert st1.state_copy_launches_in_last_plan == 0 and st1.state_copy_jobs_in_last_plan == 0
    check(generic, want, "flag 1")
    check(got, generic, "one launch against flag 1")


def test_a_run_longer_than_the_table_takes_two_launches():
    def build(g):
        c = Case(g)
        x, y = c.tensor(5, 3, 40), c.tensor(5, 3, 40)
        for b in range(40):
            c.copy((g.view_2d(c.tensors[x], 5, 3, 20, b * 60), x, b * 15, 15), (g.view_2d(c.tensors[y], 5, 3, 20, (39 - b) * 60), y, (39 - b) * 15, 15))
        return c
    got, want, st = run_case(build)
    assert st.state_copy_launches_in_last_plan == 2 and st.state_copy_jobs_in_last_plan == 40
    check(got, want, "40 jobs")


def test_a_later_job_that_reads_an_earlier_destination_stays_generic():
    def build(g):
        c = Case(g)
        x, out = c.tensor(2, 64, B), c.tensor(128)
        c.copy(c.column(x, 2, 64, 1), c.column(x, 2, 64, 2))
        c.copy(c.column(x, 2, 64, 2), c.piece(out, 2, 64, 0))        # reads what the first copy writes: two runs of one job, neither taken
        return c
    got, want, st = run_case(build)
    assert st.state_copy_launches_in_last_plan == 0 and st.kernels_in_last_plan == 2
    check(got, want, "dependent pair")


def test_a_hazard_ends_the_run_and_the_rest_is_still_right():
    def build(g):
        c = Case(g)
        x, y, out = c.tensor(5, 3, B), c.tensor(2, 64, B), c.tensor(16)
        c.copy(c.column(x, 5, 3, 1), c.column(x, 5, 3, 2))
        c.copy(c.column(y, 2, 64, 0), c.column(y, 2, 64, 1))
        c.copy(c.column(x, 5, 3, 2), c.piece(out, 5, 3, 0))          # reads job 0's destination: the run ends in front of it ...
        c.copy(c.column(y, 2, 64, 2), c.column(y, 2, 64, 0))         # ... and these two, free of each other, make a second launch behind the first
        return c
    got, want, st = run_case(build)
    assert st.state_copy_launches_in_last_plan == 2 and st.state_copy_jobs_in_last_plan == 4 and st.kernels_in_last_plan == 2
    check(got, want, "hazard")


def test_a_source_that_overlaps_its_destination_stays_generic():
    def build(g):
        c = Case(g)
        x, y, z = c.tensor(2, 64, B), c.tensor(5, 3, B), c.tensor(6, 1, B)
        c.copy(c.column(x, 2, 64, 1), c.column(x, 2, 64, 1))         # onto itself: declined, and the bytes stay what they are
        c.copy(c.column(y, 5, 3, 0), c.column(y, 5, 3, 2))
        c.copy(c.column(x, 2, 64, 0), c.column(x, 2, 64, 2))
        c.copy(c.column(z, 6, 1, 1), c.column(z, 6, 1, 0))
        return c
    got, want, st = run_case(build)
    assert st.state_copy_launches_in_last_plan == 1 and st.state_copy_jobs_in_last_plan == 3
    check(got, want, "self copy")


def test_lone_columns_and_rows_stay_generic():
    def build(g):
        c = Case(g)
        x, r = c.tensor(64, 5, B), c.tensor(64, 1, B)
        c.copy(c.column(r, 64, 1, 0), c.column(r, 64, 1, 2))         # a row of a [dim, 1, B] state (transformer_out)
        c.copy(c.column(x, 64, 5, 0), c.column(x, 64, 5, 1))         # one column of two or more rows (cond_cross): not two
        return c
    got, want, st = run_case(build)
    assert st.state_copy_launches_in_last_plan == 0 and st.kernels_in_last_plan == 2
    check(got, want, "lone column")
