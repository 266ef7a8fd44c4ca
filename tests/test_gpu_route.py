"""Every route of csrc/route.h taken on the GPU, at the smallest shape that takes it on the auto rule: the wide kernel
unplanned and planned, the 16-wave and 8-wave narrow kernels, the sorted-window, claim and claim16 forms, and the coop
form (set_kernel only); then every forced set_kernel value on one batch.  Per route: kvsep_crc32c_kernel_name names the
expected kernel, kvsep_crc32c_plan_query agrees (plan entries iff planned), the batch form equals the host CRC for every
block, and the verify form with one planted bad word reports that block and a count of one.  Offsets are
1 + i (len + 3): nothing is aligned.  None of the shapes is a workload size."""
import numpy as np
import pytest

import kvsep

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
CUS = torch.cuda.get_device_properties(0).multi_processor_count
KiB = 1024


def _uniform(count, blen):
    ln = np.full(count, blen, np.uint64)
    return np.uint64(1) + np.arange(count, dtype=np.uint64) * np.uint64(blen + 3), ln


def _ragged(count):
    """16..256 B, mean about 64, one block at the 256-B hint: 4 * 256 > 5 * mean, a ragged batch."""
    x = np.random.default_rng(20).integers(0, 241, count).astype(np.uint64)
    ln = np.uint64(16) + x * x * x // np.uint64(240 * 240)
    ln[count // 2] = 256
    off = np.uint64(1) + np.concatenate((np.zeros(1, np.uint64), np.cumsum(ln + np.uint64(3))[:-1]))
    return off, ln


# name -> (set_kernel value, expected kernel, planned, max_len hint, (off, len) builder)
SHAPES = {
    "wide": ("auto", "crc32c_pieces_kernel", False, 100, lambda: _uniform(64, 100)),
    "planned": ("auto", "crc32c_pieces_kernel", True, 0, lambda: _uniform(3, 300 * KiB + 7)),
    "narrow16": ("auto", "crc32c_narrow_kernel", False, 64, lambda: _uniform(32 * CUS, 64)),
    "sorted": ("auto", "crc32c_narrow_sorted_kernel", False, 256, lambda: _ragged(32 * CUS)),
    "claim": ("auto", "crc32c_narrow_claim_kernel", False, 64, lambda: _uniform(32768, 64)),
    "claim16": ("auto", "crc32c_narrow_claim_kernel", False, 8 * KiB, lambda: _uniform(4096, 8 * KiB)),
    "narrow8": ("auto", "crc32c_narrow_kernel", False, 16, lambda: _uniform(3 * 2**17 + 1, 16)),
    "coop": ("coop", "crc32c_narrow_coop_kernel", False, 4 * KiB, lambda: _uniform(64, 4 * KiB)),
}
# every set_kernel value on the claim shape (32,768 x 64 B)
FORCED = {"auto": "crc32c_narrow_claim_kernel", "wide": "crc32c_pieces_kernel", "narrow": "crc32c_narrow_claim_kernel",
          "narrow16": "crc32c_narrow_kernel", "narrow8": "crc32c_narrow_kernel", "sorted": "crc32c_narrow_sorted_kernel",
          "claim": "crc32c_narrow_claim_kernel", "claim16": "crc32c_narrow_claim_kernel",
          "coop": "crc32c_narrow_coop_kernel"}


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def masked(crc):
    c = crc.astype(np.uint64)
    return ((((c >> np.uint64(15)) | (c << np.uint64(17))) + np.uint64(0xA282EAD8)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = kvsep.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batches(oracle):
    """Each shape's data, descriptors and host CRCs, built once and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            off, ln = SHAPES[name][4]()
            size = int(off[-1] + ln[-1]) + 1
            data = np.random.default_rng(len(name) + size).integers(0, 256, size, dtype=np.uint8)
            crc = oracle.batch(data, off, ln, threads=8)
            cache[name] = dict(data=torch.from_numpy(data).to(DEV), off=dev_u64(off), len=dev_u64(ln), crc=crc,
                               count=len(off), total=int(ln.sum()), stored=masked(crc))
        return cache[name]

    return get


def check_route(ctx, b, max_len, kernel, planned):
    count, total = b["count"], b["total"]
    assert ctx.kernel_name(count, max_len, total) == kernel
    _, pieces, _ = ctx.plan_query(count, max_len, total)
    assert (pieces > 0) == planned, pieces
    out = torch.zeros(count, dtype=torch.int32, device=DEV)
    ctx.batch_device(b["data"].data_ptr(), b["off"], b["len"], out, count=count, total_bytes=total, max_len=max_len)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), b["crc"])
    bad = (2 * count) // 3
    stored = b["stored"].copy()
    stored[bad] ^= 0x10000
    out.zero_()
    fb = torch.zeros(1, dtype=torch.int64, device=DEV)
    nb = torch.zeros(1, dtype=torch.int64, device=DEV)
    ctx.verify_device(b["data"].data_ptr(), b["off"], b["len"], dev_u32(stored), out, fb, nb, count=count,
                      total_bytes=total, max_len=max_len)
    torch.cuda.synchronize()
    assert (fb.item(), nb.item()) == (bad, 1)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), b["crc"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_each_route_at_its_smallest_shape(ctx, batches, name):
    setting, kernel, planned, max_len, _ = SHAPES[name]
    ctx.set_kernel(setting)
    try:
        check_route(ctx, batches(name), max_len, kernel, planned)
    finally:
        ctx.set_kernel("auto")


@pytest.mark.parametrize("setting", list(FORCED))
def test_each_forced_kernel(ctx, batches, setting):
    assert set(FORCED) == set(kvsep.Context.KERNELS)
    ctx.set_kernel(setting)
    try:
        check_route(ctx, batches("claim"), 64, FORCED[setting], False)
    finally:
        ctx.set_kernel("auto")
