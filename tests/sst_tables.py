"""A small SST table writer and a plain index-block parser -- TEST INFRASTRUCTURE for the SST table reader's tests
(test_sst_index_cpu.py, test_gpu_sst_table.py, test_isa_envelope_sst.py).  The writer lays out what the reference's
TableBuilder lays out (table/table_builder.cc, table/block_builder.cc, table/format.cc): data blocks with their 5-byte
trailers, an empty metaindex block, an index block at any restart interval, the 48-byte footer.
test_sst_index_cpu.py pins it to the reference's format: fed the keys and handles of tests/golden/ref_table.sst's index
block it reproduces that block byte for byte."""
import numpy as np

import kvsep

MAGIC = 0xdb4775248b80fb57


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def get_varint(b, p: int, limit: int, maxbytes: int = 10):
    v = 0
    for i in range(maxbytes):
        if p >= limit:
            break
        byte = b[p]
        p += 1
        v |= (byte & 127) << (7 * i)
        if byte < 128:
            return v, p
    raise ValueError("bad varint")


def handle_bytes(off: int, ln: int) -> bytes:
    return varint(off) + varint(ln)


def index_block(keys, handles, interval: int = 1) -> bytes:
    """BlockBuilder::Add for every (key, handle value) and Finish(): prefix-compressed entries, a restart point every
    `interval` entries, the restart array and its count."""
    buf = bytearray()
    restarts = [0]
    last = b""
    counter = 0
    for key, (off, ln) in zip(keys, handles):
        shared = 0
        if counter < interval:
            m = min(len(last), len(key))
            while shared < m and last[shared] == key[shared]:
                shared += 1
        else:
            restarts.append(len(buf))
            counter = 0
        val = handle_bytes(off, ln)
        buf += varint(shared) + varint(len(key) - shared) + varint(len(val)) + key[shared:] + val
        last = key
        counter += 1
    for r in restarts:
        buf += int(r).to_bytes(4, "little")
    buf += len(restarts).to_bytes(4, "little")
    return bytes(buf)


def parse_index(block: bytes):
    """Block::Iter from SeekToFirst to the end, keys included -> (keys, [(off, len)])."""
    n = len(block)
    nr = int.from_bytes(block[n - 4:n], "little")
    ro = n - 4 * (1 + nr)
    keys, handles, key, p = [], [], b"", 0
    while p < ro:
        shared, p = get_varint(block, p, ro, 5)
        non_shared, p = get_varint(block, p, ro, 5)
        vlen, p = get_varint(block, p, ro, 5)
        key = key[:shared] + bytes(block[p:p + non_shared])
        v = p + non_shared
        off, q = get_varint(block, v, v + vlen)
        ln, q = get_varint(block, q, v + vlen)
        keys.append(key)
        handles.append((off, ln))
        p = v + vlen
    return keys, handles


def trailer(block: bytes, type_byte: int = 0) -> bytes:
    """[type][Mask(Value(block || type)) LE32] (table/table_builder.cc:209-232)."""
    crc = kvsep.extend(kvsep.value(block), bytes([type_byte]))
    return bytes([type_byte]) + kvsep.mask(crc).to_bytes(4, "little")


def footer(meta, index) -> bytes:
    f = handle_bytes(*meta) + handle_bytes(*index)
    return f + bytes(40 - len(f)) + MAGIC.to_bytes(8, "little")


def key_of(i: int) -> bytes:
    return b"key%010d" % i + (i * 256 + 1).to_bytes(8, "little")  # a user key and an 8-byte sequence / type tag


def build_table(nblocks: int, interval: int = 1, block_len=None, seed: int = 1):
    """-> (image uint8 array, off, len, (meta_off, meta_len), (index_off, index_len)): nblocks data blocks of
    block_len(i) pseudo-random bytes (default 40..200), the empty metaindex block, the index block, the footer."""
    rng = np.random.default_rng(seed)
    lens = [int(block_len(i)) if block_len else int(rng.integers(40, 201)) for i in range(nblocks)]
    parts, off, p = [], [], 0
    payload = kvsep.splitmix64_bytes(sum(lens) + 8, seed, 0).tobytes()
    q = 0
    for ln in lens:
        blk = payload[q:q + ln]
        q += ln
        off.append(p)
        parts += [blk, trailer(blk)]
        p += ln + 5
    meta_blk = index_block([], [], 1)  # one restart point, no entry: 8 bytes
    meta = (p, len(meta_blk))
    parts += [meta_blk, trailer(meta_blk)]
    p += len(meta_blk) + 5
    idx_blk = index_block([key_of(i) for i in range(nblocks)], list(zip(off, lens)), interval)
    index = (p, len(idx_blk))
    parts += [idx_blk, trailer(idx_blk), footer(meta, index)]
    img = np.frombuffer(b"".join(parts), np.uint8).copy()
    return img, np.array(off, np.uint64), np.array(lens, np.uint64), meta, index
