"""What zsw_prune_rescored counts (include/zoe_sw.h): the reads the FORWARD seeded pass handed back and that were scored over all
their cells — for every entry point of the read-as-profile role, also those that run a second, reversed seeded pass (ranges,
alignment, 3-pass alignment), whose unsettled reads are not rescored and must not be counted.

The witness is independent of the counter: zsw_debug_band_records is written by the forward pass only, a later tier overwrites an
earlier one, and bit 0 of record [7] says "accepted by this walk". With the records zero-filled before the call, the reads handed
back are those whose bit is 0. The plain score call checks the witness itself (one seeded pass, nothing else to count)."""
import ctypes as C

import numpy as np
import pytest

import abi_helpers as ah

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests need an MI355X")
    import zoe_amd
    from zoe_amd import _lib, synth

    ref = synth.reference_host(2000)
    rng = np.random.default_rng(812)
    r = np.frombuffer(ref, dtype=np.uint8)
    n, L = 6000, 150
    # 3 % to 12 % substitutions, every other read with an indel, and a few unrelated reads: the forward pass hands back a good
    # part of them, and of those it keeps the reversed pass (other k-mers, other bounds) hands back some more
    reads = [ah._one_read(rng, r, L, "diverged" if i % 25 else "random", i)[0] for i in range(n)]
    rs = ah.ReadSet("diverged", ref, reads, L, np.zeros(n, dtype=np.int64), np.full(n, -1))
    lib = _lib.load()
    dna = zoe_amd.WeightMatrix.new_dna_matrix(2, -5, b"N")
    h = ah.new_context(_lib, lib, dna, -10, -1, ref, pseq=ref)
    yield _lib, lib, h, rs
    lib.zsw_destroy(h)


def _rescored(lib, h):
    v = C.c_uint64(0)
    assert lib.zsw_prune_rescored(h, C.byref(v)) == 0
    return int(v.value)


@pytest.mark.parametrize("entry_name", ["zsw_score_batch_from", "zsw_score_ranges_batch", "zsw_align_batch_from", "zsw_align_3pass_batch_from"])
def test_rescored_is_the_forward_passs_handbacks(world, entry_name):
    import torch

    _lib, lib, h, rs = world
    n = rs.n
    p = ah.Presented(_lib, rs, "device-fixed")
    rec = torch.zeros(8 * n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.zsw_debug_band_records(h, rec.data_ptr()) == 0
    try:
        res = ah.Call(_lib, lib, h, ah.ENTRY[entry_name], p).run().collect()
        back = _rescored(lib, h)
    finally:
        assert lib.zsw_debug_band_records(h, None) == 0
    accepted = int((rec.cpu().numpy().reshape(n, 8)[:, 7] & 1).sum())
    print(f"{entry_name}: zsw_prune_rescored {back}, band records: {accepted} of {n} accepted, {int((res['status'] == 0).sum())} reads with a score")
    assert 0 < accepted < n
    assert back == n - accepted


@pytest.mark.parametrize("entry_name,counts", [("zsw_score_shared_batch_from", True), ("zsw_score_ends_shared_batch", False),
                                               ("zsw_score_ranges_shared_batch_from", False), ("zsw_align_3pass_shared_batch_from", False)])
def test_rescored_in_the_shared_role(world, entry_name, counts):
    """shared role: the score calls count the hand-backs of the role-swapped pass (the same reads as the read role's score call:
    the pass, its index and its bounds are those of the read role with the matrix transposed, which is symmetric here); the ends,
    ranges and alignment calls rescore nothing — a read handed back joins the reads with ties under the shared role's own
    kernel — and report 0."""
    _lib, lib, h, rs = world
    p = ah.Presented(_lib, rs, "device-fixed")
    ah.Call(_lib, lib, h, ah.ENTRY["zsw_score_batch_from"], p).run().collect()
    read_role = _rescored(lib, h)
    ah.Call(_lib, lib, h, ah.ENTRY[entry_name], p).run().collect()
    back = _rescored(lib, h)
    assert back == (read_role if counts else 0), (back, read_role)
