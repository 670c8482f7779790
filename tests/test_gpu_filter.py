"""GPU `zsw_sneaky_snake_batch` against the oracle's restatement of sneaky_snake (sneaky_snake.rs:78-131): same
Some(true) / Some(false) / None for every (reference window, read) pair."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CODE = {False: 0, True: 1, None: 2}


@pytest.fixture(scope="module")
def za():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd

    return zoe_amd


def test_doc_example(za):
    # sneaky_snake.rs:55-60
    out = za.sneaky_snake(b"GGTGCAGAGCTC", [b"GGTGAGAGTTGT"], [0], [12], 0.25)
    assert out.cpu().tolist() == [1]


def mutate(rng, s, n_edits):
    s = s.copy()
    for _ in range(n_edits):
        k = int(rng.integers(0, 3))
        p = int(rng.integers(0, max(1, len(s))))
        if k == 0 and len(s):
            s[p] = rng.choice(list(b"ACGT"))
        elif k == 1 and len(s) > 1:
            s = np.delete(s, p)
        else:
            s = np.insert(s, p, rng.choice(list(b"ACGT")))
    return s.astype(np.uint8)


@pytest.mark.parametrize("thr", [0.0, 0.04, 0.1, 0.25, 0.5, 1.0, 1.5])
def test_random_windows_vs_oracle(za, oracle, thr):
    rng = np.random.default_rng(int(thr * 1000) + 3)
    ref = rng.choice(list(b"ACGT"), 3000).astype(np.uint8)
    reads, rs, rl = [], [], []
    for i in range(700):
        L = int(rng.integers(1, 260))
        st = int(rng.integers(0, len(ref) - L))
        if i % 50 == 0:
            st = len(ref) - L  # window touching the end of the reference
        if i % 50 == 1:
            st = 0
        q = mutate(rng, ref[st:st + L], int(rng.integers(0, 1 + L // 6)))
        if i % 9 == 0:
            q = rng.choice(list(b"ACGT"), L).astype(np.uint8)  # unrelated
        wl = int(np.clip(L + rng.integers(-3, 4), 0, len(ref) - st))
        if len(q) == 0:
            q = np.frombuffer(b"A", dtype=np.uint8)
        reads.append(q.tobytes())
        rs.append(st)
        rl.append(wl)
    got = za.sneaky_snake(ref.tobytes(), reads, rs, rl, thr).cpu().numpy()
    want = np.array([CODE[oracle.sneaky_snake(ref[s:s + l].tobytes(), q, thr)] for q, s, l in zip(reads, rs, rl)], dtype=np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    if 0.0 < thr < 1.0:
        assert len(set(want.tolist())) >= 2


def test_fixed_length_device_batch_and_host_batch(za, oracle):
    import ctypes as C
    import torch

    from zoe_amd import _lib, synth

    R, L, n = 2000, 150, 4096
    ref = synth.reference_host(R)
    ctx = za.SwContext.get(0)
    reads = synth.reads_device(ctx, ref, 0, n, L)
    host = reads.bases.cpu().numpy().reshape(n, L)
    # candidate window = where the read was drawn from is unknown to the filter: use the score-ranges start instead
    m = za.WeightMatrix.new_dna_matrix(2, -5, b"N")
    rg = za.StripedProfileBatch(reads, m, -10, -1, T="i16", N=16).sw_score_ranges(za.SeqSrc.Reference(ref))
    st = np.clip(rg.ref_start.cpu().numpy().astype(np.int64) - rg.query_start.cpu().numpy().astype(np.int64), 0, R - L)
    ln = np.full(n, L)
    got = za.sneaky_snake(ref, reads, st, ln, 0.05).cpu().numpy()
    want = np.array([CODE[oracle.sneaky_snake(ref[s:s + L], host[i].tobytes(), 0.05)] for i, s in enumerate(st)], dtype=np.uint8)
    assert np.array_equal(got, want)
    assert 0.5 < (got == 1).mean() < 1.0  # most 1 %-error reads pass at 5 %, the random ones do not

    # the same batch through host pointers
    lib = _lib.load()
    b = _lib.ZswBatch()
    flat = np.ascontiguousarray(host.reshape(-1))
    b.bases, b.offsets, b.fixed_len, b.n_reads, b.mem = flat.ctypes.data, None, L, n, _lib.MEM_HOST
    st32, ln32 = st.astype(np.uint32), ln.astype(np.uint32)
    out = np.zeros(n, dtype=np.uint8)
    rc = lib.zsw_sneaky_snake_batch(ctx.h, C.byref(b), st32.ctypes.data, ln32.ctypes.data, C.c_float(0.05), out.ctypes.data, None)
    assert rc == 0 and np.array_equal(out, want)
    # a window that leaves the reference: error for host arrays, 255 for device arrays
    st32[7] = R - 10
    assert lib.zsw_sneaky_snake_batch(ctx.h, C.byref(b), st32.ctypes.data, ln32.ctypes.data, C.c_float(0.05), out.ctypes.data, None) == -1
    bad = za.sneaky_snake(ref, reads, st32.astype(np.int64), ln, 0.05).cpu().numpy()
    assert bad[7] == 255 and np.array_equal(np.delete(bad, 7), np.delete(want, 7))
    torch.cuda.synchronize()


def _host_batch(_lib, flat, n, fixed_len=0, offsets=None, encoding=0, mem=None):
    b = _lib.ZswBatch()
    b.bases, b.offsets, b.fixed_len, b.n_reads = flat.ctypes.data, (None if offsets is None else offsets.ctypes.data), fixed_len, n
    b.mem, b.encoding = (_lib.MEM_HOST if mem is None else mem), encoding
    return b


def test_packed_and_unknown_encodings_are_rejected(za, oracle):
    """The filter compares raw bytes, so a ZSW_ENCODING_PACKED4 batch has no meaning for it: ZSW_ERR_INVALID_ARGUMENT with a
    message, for host and device batches, before anything is copied or written; so is an unknown encoding, and so are host
    offsets that go backwards. The context filters correctly afterwards. (The packed buffer is allocated at the full n * L
    bytes: a library that took it for bytes would read inside it and return verdicts, which the assertion on rc catches.)"""
    import ctypes as C
    import torch

    from zoe_amd import _lib, synth

    R, L, n = 2000, 151, 1024
    ref = synth.reference_host(R)
    ctx = za.SwContext.get(0)
    ctx.set_scoring(za.WeightMatrix.new_dna_matrix(2, -5, b"N"), -10, -1)
    ctx.set_reference(ref)
    lib = _lib.load()
    rng = np.random.default_rng(5)
    st = rng.integers(0, R - L, n).astype(np.uint32)
    ln = np.full(n, L, dtype=np.uint32)
    r = np.frombuffer(ref, dtype=np.uint8)
    reads = np.ascontiguousarray([np.resize(mutate(rng, r[s:s + L], int(rng.integers(0, 12))), L) if i % 3 else rng.choice(list(b"ACGT"), L).astype(np.uint8)
                                  for i, s in enumerate(st)], dtype=np.uint8)
    want = np.array([CODE[oracle.sneaky_snake(ref[s:s + L], reads[i].tobytes(), 0.05)] for i, s in enumerate(st)], dtype=np.uint8)
    assert len(set(want.tolist())) >= 2
    flat = reads.reshape(-1)
    packed = np.zeros(n * L, dtype=np.uint8)  # room for n * L bytes; the packed reads fill the first n * 76
    assert lib.zsw_pack4_host(ctx.h, flat.ctypes.data, n, L, packed.ctypes.data) == 0
    msg = lambda: lib.zsw_last_error_string(ctx.h).decode()
    call = lambda b, out: lib.zsw_sneaky_snake_batch(ctx.h, C.byref(b), st.ctypes.data, ln.ctypes.data, C.c_float(0.05), out.ctypes.data, None)
    out = np.full(n, 0xA5, dtype=np.uint8)
    assert call(_host_batch(_lib, packed, n, L, encoding=1), out) == -1 and "encoding" in msg()
    assert (out == 0xA5).all()
    assert call(_host_batch(_lib, flat, n, L, encoding=7), out) == -1 and "encoding" in msg()
    assert (out == 0xA5).all()
    # a device batch: the same answer, nothing launched
    d_bases, d_st, d_ln = torch.from_numpy(packed).cuda(), torch.from_numpy(st.view(np.int32)).cuda(), torch.from_numpy(ln.view(np.int32)).cuda()
    d_out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    bd = _lib.ZswBatch()
    bd.bases, bd.offsets, bd.fixed_len, bd.n_reads, bd.mem, bd.encoding = d_bases.data_ptr(), None, L, n, _lib.MEM_DEVICE, 1
    assert lib.zsw_sneaky_snake_batch(ctx.h, C.byref(bd), d_st.data_ptr(), d_ln.data_ptr(), C.c_float(0.05), d_out.data_ptr(), None) == -1 and "encoding" in msg()
    torch.cuda.synchronize()
    assert bool((d_out == 0xA5).all())
    # host offsets that go backwards (inside the buffer)
    offs = (np.arange(n + 1, dtype=np.uint64) * L)
    offs[n // 2] += 2 * L
    assert call(_host_batch(_lib, flat, n, 0, offsets=offs), out) == -1 and "monotone" in msg()
    assert (out == 0xA5).all()
    # the context still filters
    assert call(_host_batch(_lib, flat, n, L), out) == 0 and np.array_equal(out, want)
    bd.bases, bd.encoding = torch.from_numpy(flat).cuda().data_ptr(), 0
    assert lib.zsw_sneaky_snake_batch(ctx.h, C.byref(bd), d_st.data_ptr(), d_ln.data_ptr(), C.c_float(0.05), d_out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)


def test_ragged_host_batch_equals_ragged_device_batch(za, oracle):
    """Ragged reads through host pointers (offsets in host memory): the oracle's verdicts, and those of the ragged device batch."""
    import ctypes as C

    from zoe_amd import _lib

    rng = np.random.default_rng(2026)
    ref = rng.choice(list(b"ACGT"), 3000).astype(np.uint8)
    reads, rs, rl = [], [], []
    for i in range(2500):
        L = int(rng.integers(1, 300))
        st = int(rng.integers(0, len(ref) - L))
        q = mutate(rng, ref[st:st + L], int(rng.integers(0, 1 + L // 8)))
        if i % 7 == 0:
            q = rng.choice(list(b"ACGT"), L).astype(np.uint8)
        if i % 101 == 0:
            q = np.zeros(0, dtype=np.uint8)  # an empty read
        reads.append(q.tobytes())
        rs.append(st)
        rl.append(int(np.clip(L + rng.integers(-2, 3), 0, len(ref) - st)))
    thr = 0.06
    want = np.array([CODE[oracle.sneaky_snake(ref[s:s + l].tobytes(), q, thr)] for q, s, l in zip(reads, rs, rl)], dtype=np.uint8)
    assert set(want.tolist()) == {0, 1, 2}
    dev = za.sneaky_snake(ref.tobytes(), reads, rs, rl, thr).cpu().numpy()
    ctx = za.SwContext.get(0)
    flat = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(q) for q in reads], out=offs[1:])
    st32, ln32 = np.array(rs, dtype=np.uint32), np.array(rl, dtype=np.uint32)
    guard = 64
    buf = np.full(len(reads) + 2 * guard, 0xA5, dtype=np.uint8)
    b = _host_batch(_lib, flat, len(reads), 0, offsets=offs)
    rc = _lib.load().zsw_sneaky_snake_batch(ctx.h, C.byref(b), st32.ctypes.data, ln32.ctypes.data, C.c_float(thr), buf.ctypes.data + guard, None)
    assert rc == 0
    assert (buf[:guard] == 0xA5).all() and (buf[-guard:] == 0xA5).all()
    host = buf[guard:-guard]
    bad = np.nonzero(host != want)[0]
    assert bad.size == 0, (bad[:5], host[bad[:5]], want[bad[:5]])
    assert np.array_equal(dev, host)
