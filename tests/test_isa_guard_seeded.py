"""The seeded twin of the headline's renderC kernel (csrc/psdr_kernels.h k_camera_seeded: the slots' PCG32 seeds come from the handle's seed table) exists in the
built library, is SHORTER than its twin -- the two TEA mixes are what it is there to leave out -- and brings no scratch instruction of its own (the twin sits on a spill
cliff at 80 VGPRs).  The twin in the same build is the yardstick: no table.  Disassembly as in tests/test_isa_guard.py.  CPU test."""
import pytest

import test_isa_guard

TWINS = {
    "k_camera_seeded<float, float, 1, 8, true>": "k_camera<float, float, 1, 8, true>",
}


@pytest.fixture(scope="module")
def counts():
    saved = test_isa_guard.KERNELS
    test_isa_guard.KERNELS = dict(saved, **{k: "seeded twin of " + v for k, v in TWINS.items()})
    try:
        return test_isa_guard.disassemble()
    finally:
        test_isa_guard.KERNELS = saved


@pytest.mark.parametrize("seeded", sorted(TWINS))
def test_seeded_kernel_is_shorter_than_its_twin_and_spills_no_more(counts, seeded):
    twin = TWINS[seeded]
    assert seeded in counts, "%s not found in the library" % seeded
    assert twin in counts
    a, b = counts[seeded], counts[twin]
    print("%s: %d instructions / %d scratch; %s: %d / %d" % (seeded, a["instructions"], a["scratch"], twin, b["instructions"], b["scratch"]))
    assert a["instructions"] < b["instructions"]
    assert a["scratch"] <= b["scratch"]
