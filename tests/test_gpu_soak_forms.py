"""Seeded differential soak of the device forms built since round 6 (kv-separate_amd/tools/soak_forms.py, a fixed
slice): the list forms, concat and gather, pack and the vlog / SST frame forms, the offsets pass and the two salvage
forms, the log walk / read / accept-gaps / chains / records forms over images with up to five damages, the log frame
form and the device reader over its output, the SST index walk, table verify and keys walk over damaged tables at
restart intervals 1, 2 and 16, the index block build, table finish and table rewrite -- random counts around the 64-lane, 256-lane and
1,024-tile edges, any source and destination skew, keep masks, caps below / at / above, destinations one byte short --
and mixed sequences of them on one fresh context: across two streams with no host step, and captured into one graph that
is replayed over inputs rewritten in place (and one call captured over its reservation, which must write nothing).  Every output element, destination byte, guard and input is compared with a
plain serial model over the oracle's CRC (never the host forms: they share the kernels' rule headers); one case runs
once, a test stops at its first mismatch, and the failing case is rebuilt alone from its printed family/seed/case.
tests/test_soak_forms_cpu.py checks the models, the generators' reach at these counts and the comparator."""
import os
import sys

import pytest

import kvsep

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kv-separate_amd", "tools"))
import soak_forms as S  # noqa: E402
from soak_forms_counts import CASES, SEEDS  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("family", S.FAMILIES)
def test_seeded_forms_soak(ctx, family, seed):
    elements = 0
    for k in range(CASES[family]):
        c = S.make_case(family, seed, k)
        S.check_case(ctx, c)
        elements += c.elements
    print(f"{family}/{seed}: {CASES[family]} cases, {elements} elements")
