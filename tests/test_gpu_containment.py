"""Where the kernels write, on the hardware: out[0 .. count), first_bad and nbad, and nothing else.

The result words are carved from the interior of a larger tensor, 256 B of 0xA5 canaries on each side of each; every
forced kernel form (kvsep_crc32c_ctx_set_kernel), plain and verify, eager, at counts of one block, one group and a
block, one sorted window and a block, four windows and a block.  After each call the canaries are intact, the payload
equals its clone and the results equal the oracle.

The payload keeps the usual padding and no block lies at the edge of an allocation: what the kernels READ is checked
on the CPU, by emulating the shipped assembly with every byte's accesses marked (tests/test_isa_envelope.py) -- on
the hardware a read outside a mapping would be a fault, not a failed assertion.  Needs a gfx950 device (`-m gpu`).
"""
import numpy as np
import pytest

import kvsep
from kvsep import splitmix64_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
CANARY, MARGIN = 0xA5, 256
N = 257
KERNEL_NAME = {"wide": "pieces", "narrow16": "narrow_kernel", "narrow8": "narrow_kernel", "sorted": "sorted",
               "claim": "claim", "claim16": "claim", "coop": "coop"}


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch(oracle):
    """257 ragged blocks of 0 .. 1500 B at every start alignment, 64 B apart at least, 4 KiB from either end of the
    payload's tensor; the oracle's CRCs (with inits), once."""
    rng = np.random.default_rng(20261019)
    ln = rng.integers(0, 1501, N).astype(np.uint64)
    ln[:4] = [129, 0, 1500, 1]
    gap = (64 + rng.integers(0, 128, N)).astype(np.uint64)
    off = np.full(N, 4096, np.uint64)
    off[1:] += np.cumsum(ln[:-1] + gap[:-1], dtype=np.uint64)
    host = splitmix64_bytes(int(off[-1] + ln[-1]) + 4096, 77, 0)
    init = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32)
    exp = oracle.batch(host, off, ln, init, threads=8)
    stored = np.array([oracle.lib.oracle_crc32c_mask(int(c)) for c in exp], np.uint32)
    bad = np.array([0, 8, 64, 200, 256])  # planted mismatches: whichever of them a count includes
    stored[bad] ^= 0x100
    d = torch.from_numpy(host).to(DEV)
    t = lambda a, v: torch.from_numpy(np.ascontiguousarray(a).view(v)).to(DEV)
    return dict(d=d, clone=d.clone(), off=t(off, np.int64), ln=t(ln, np.int64), init=t(init, np.int32),
                stored=t(stored, np.int32), lens=ln, exp=exp, bad=bad)


def carve(count, verify):
    """A canary-filled arena with out[count] (and first_bad, nbad) inside it, MARGIN canary bytes around each.
    -> (arena, {name: (byte offset, bytes)})"""
    spans = {"out": (MARGIN, 4 * count)}
    end = MARGIN + 4 * count
    if verify:
        for name in ("first_bad", "nbad"):
            o = (end + MARGIN + 7) // 8 * 8
            spans[name] = (o, 8)
            end = o + 8
    arena = torch.full((end + MARGIN,), CANARY, dtype=torch.uint8, device=DEV)
    return arena, spans


@pytest.mark.parametrize("verify", [False, True], ids=["plain", "verify"])
@pytest.mark.parametrize("count", [1, 9, 65, 257])
@pytest.mark.parametrize("kernel", list(KERNEL_NAME))
def test_writes_stay_inside_the_result_words(ctx, batch, kernel, count, verify):
    b = batch
    ctx.set_kernel(kernel)
    max_len = max(int(b["lens"][:count].max()), 1)
    total = int(b["lens"][:count].sum())
    assert KERNEL_NAME[kernel] in ctx.kernel_name(count, max_len, total)
    arena, spans = carve(count, verify)
    ptr = {k: arena.data_ptr() + o for k, (o, _) in spans.items()}
    args = dict(init=b["init"], count=count, total_bytes=total, max_len=max_len)
    if verify:
        ctx.verify_device(b["d"].data_ptr(), b["off"], b["ln"], b["stored"], ptr["out"], ptr["first_bad"],
                          ptr["nbad"], **args)
    else:
        ctx.batch_device(b["d"].data_ptr(), b["off"], b["ln"], ptr["out"], **args)
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    inside = np.zeros(got.size, bool)
    for o, n in spans.values():
        inside[o:o + n] = True
    hit = np.nonzero(~inside & (got != CANARY))[0]
    assert hit.size == 0, f"{kernel}: canary bytes written at arena offsets {hit[:8]} (carved: {spans})"
    assert torch.equal(b["d"], b["clone"]), f"{kernel}: the payload was written"
    o, n = spans["out"]
    assert np.array_equal(got[o:o + n].copy().view(np.uint32), b["exp"][:count])
    if verify:
        bad = b["bad"][b["bad"] < count]
        fb = int(got[spans["first_bad"][0]:][:8].copy().view(np.int64)[0])
        nb = int(got[spans["nbad"][0]:][:8].copy().view(np.int64)[0])
        assert (fb, nb) == (int(bad.min()), bad.size)
