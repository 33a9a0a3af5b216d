"""The device layout of a fixed list of small configurations, pinned array by array (tools/layout_digest.py, CPU only).

build_layout's output is data: every rule, threshold and tie-break of csrc/layout.cpp ends up in the arrays of the checkpoint format.  The
golden file holds, per configuration, 48 bits of the SHA-256 of each array (ids 1-39 of layout.hpp's LAY_* enum), of the bddmma_layout_size
values, of narrow_words and of slot_to_instr (one string, in the order of layout_digest.ITEMS), so a change of a rule shows which arrays of
which configurations moved — and a refactor shows none.
After a deliberate change: python tools/layout_digest.py --small --write."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import layout_digest  # noqa: E402

with open(layout_digest.GOLDEN) as f:
    PINNED = json.load(f)


@pytest.fixture(scope="module")
def digests():
    return {name: dict(lines) for name, lines in layout_digest.run(small_only=True)}


def test_the_golden_file_pins_every_small_configuration(digests):
    assert sorted(digests) == sorted(PINNED)
    assert all(len(d) == 39 + 3 for d in digests.values())


@pytest.mark.parametrize("name", sorted(PINNED))
def test_layout_arrays_are_the_pinned_ones(digests, name):
    n = layout_digest.PIN_HEX
    assert len(PINNED[name]) == n * len(layout_digest.ITEMS)
    moved = [what for k, what in enumerate(layout_digest.ITEMS) if digests[name][what][:n] != PINNED[name][k * n:(k + 1) * n]]
    assert not moved, f"{name}: these arrays differ from tests/golden/layout_digests.json: {moved}"


def test_the_layout_does_not_depend_on_the_thread_count(digests, monkeypatch):
    monkeypatch.setenv("BDDMMA_THREADS", "3")
    for name, lines in layout_digest.run(small_only=True, names={"pack/uniform_runs/auto", "family/mixed/r4", "groups/long_bdds/wpb0", "bins/by_variable"}):
        assert dict(lines) == digests[name], name
