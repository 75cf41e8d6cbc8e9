"""PFACX_caseMatchFromDevice / PFACX_casePairsFromDevice / PFACX_caseMatchFromHost (GPU platform) against the references of tests/case_ref.py: the
table of the host file through the device form and the pairs form, the compare edges with the input pointer 0 - 3 bytes off a 256-byte boundary
and a match as the buffer's last bytes, pair counts around the frame's block, one list past a single grid pass, pair lists with ids and positions
that must be ignored, unsorted lists, truncation, overlapping arrays, the table accounting, and a seeded random set of 2 000 patterns of mixed
flags over 1 MiB.  All arrays are poisoned and carry guard words on both sides."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import allmatch_ref as am  # noqa: E402
from tests import case_ref as ref  # noqa: E402
from tests.case_ref import test_the_references_agree_on_every_case  # noqa: E402,F401  (runs here too: case_ref.py is not collected)
from tests.spans_ref import fold  # noqa: E402

ALL = api.PFACX_CASE_ALL
NOCASE = api.PFACX_READ_NOCASE
BLOCK = api.PFACX_CASE_BLOCK                    # scan_case.hip: kCaseBlock
PER_CU = api.PFACX_CASE_BLOCKS_PER_CU           # scan_passes.h: offsetBlocks takes eight blocks per compute unit at most
GUARD = 64
POISON = -5
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED


def text_of(pats):
    return b"".join(bytes(p) + b"\n" for p in pats)


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def gpu_handle(pats, flags=NOCASE):
    h = api.PFAC.create()
    h.readPatternFromMemoryEx(text_of(pats), flags)
    return h


def out_arrays(cap):
    return tuple(torch.full((GUARD + cap + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))


def check_guards(arrays, cap, clean_from):
    """nothing in front of the arrays, at or behind capacity, or in [clean_from, capacity)"""
    for a in arrays:
        assert bool((a[:GUARD] == POISON).all()) and bool((a[GUARD + cap:] == POISON).all()), "wrote outside the arrays"
        assert bool((a[GUARD + clean_from:GUARD + cap] == POISON).all()), "wrote behind the list"


def device_input(data, in_offset=0):
    """the input `in_offset` bytes into a tensor that ENDS with its last byte (torch allocations are 256-byte aligned) -> (tensor, address)"""
    data = as_array(data)
    host = np.full(in_offset + data.size, 0x61, dtype=np.uint8)
    host[in_offset:] = data
    d = torch.from_numpy(host).to("cuda:0")
    assert d.data_ptr() % 256 == 0
    return d, d.data_ptr() + in_offset


def device_case(cs, data, flags, in_offset=0, capacity=None, keep_on_device=False):
    """match_device -> (status, (pos, ids) of the pairs written, the full length).  The arrays take the scan's unordered list below `size`; behind
    max(size, the list) and outside the arrays nothing may be written, and the input must stay untouched"""
    data = as_array(data)
    n = int(data.size)
    cap = n * max(1, cs.max_matches_per_position) if capacity is None else capacity
    d_in, address = device_input(data, in_offset)
    before = d_in.clone()
    d_ids, d_pos = out_arrays(cap)
    st, total = cs.match_device(address, n, flags, d_ids.data_ptr() + 4 * GUARD, d_pos.data_ptr() + 4 * GUARD, cap, check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > cap), (st, total, cap)
    k = min(total, cap)
    check_guards((d_ids, d_pos), cap, min(cap, max(k, n)))
    assert torch.equal(d_in, before), "the caller's input was modified"
    pos, ids = d_pos[GUARD:GUARD + k], d_ids[GUARD:GUARD + k]
    return st, ((pos, ids) if keep_on_device else (pos.cpu().numpy(), ids.cpu().numpy())), total


def device_pairs(cs, address, n, flags, pair_ids, pair_pos, capacity):
    """pairs_device over a pair list on the host, guard words around the pair arrays too -> (status, (pos, ids), the full length)"""
    lists = []
    for a in (pair_ids, pair_pos):
        t = torch.full((GUARD + len(a) + GUARD,), POISON, dtype=torch.int32, device="cuda:0")
        t[GUARD:GUARD + len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
        lists.append(t)
    before = [t.clone() for t in lists]
    d_ids, d_pos = out_arrays(capacity)
    st, total = cs.pairs_device(address, n, flags, lists[0].data_ptr() + 4 * GUARD, lists[1].data_ptr() + 4 * GUARD, len(pair_ids),
                                d_ids.data_ptr() + 4 * GUARD if capacity else None, d_pos.data_ptr() + 4 * GUARD if capacity else None, capacity,
                                check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    check_guards((d_ids, d_pos), capacity, k)
    assert all(torch.equal(t, b) for t, b in zip(lists, before)), "the caller's pair list, or what lies around it, was modified"
    return st, (d_pos[GUARD:GUARD + k].cpu().numpy(), d_ids[GUARD:GUARD + k].cpu().numpy()), total


def longest_pairs(h, address, n):
    """the ordered longest pairs of the caseless handle: what the pairs form takes"""
    d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
    _, count = h.matchFromDeviceReduce(address, n, d_ids.data_ptr(), d_pos.data_ptr())
    torch.cuda.synchronize()
    return d_ids[:count].cpu().numpy(), d_pos[:count].cpu().numpy()


def pairs_by_definition(pair_ids, pair_pos, pats, sens, data, all_matches):
    """the contract of the pairs form, pair by pair: an id outside [1, F] or a position outside [0, n) gives nothing; the chain of the folded set from
    the pair's id down, each member that fits the buffer through the distinct patterns of its class, highest id first: a caseless one holds (that the
    folded bytes are there is the caller's business), a sensitive one where the bytes are its own"""
    folded = [fold(p) for p in pats]
    prefix, chain, _ = am.prefix_table(folded)
    variants = {}
    for (s, text), pid in ref.distinct_patterns(pats, sens).items():
        variants.setdefault(fold(text), []).append((pid, s, text))
    raw, n = bytes(data), len(data)
    pos, ids = [], []
    for q, p in zip(pair_ids.tolist(), pair_pos.tolist()):
        if not (1 <= q <= len(pats) and 0 <= p < n):
            continue
        done = False
        for _ in range(max(1, int(chain[q]))):
            if q < 1 or done:
                break
            text = folded[q - 1]
            if p + len(text) <= n and chain[q] > 0:
                for pid, s, exact in sorted(variants[text], reverse=True):
                    if not s or raw[p:p + len(exact)] == exact:
                        pos.append(p)
                        ids.append(pid)
                        done = not all_matches
                        if done:
                            break
            q = int(prefix[q])
    return np.array(pos, dtype=np.int32), np.array(ids, dtype=np.int32)


# ---------------------------------------------------------------- the cases of the host file


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_on_the_device_form_the_pairs_form_and_the_host_form(case):
    name, pats, sens, data = case
    n = len(data)
    h = gpu_handle(pats)
    try:
        with h.caseOpen(text_of(pats), ref.flags_by_id(sens)) as cs:
            assert cs.max_matches_per_position == ref.max_per_position(pats, sens)
            d_in, address = device_input(data)
            pair_ids, pair_pos = longest_pairs(h, address, n)
            for flags in (0, ALL):
                want = ref.case_brute(pats, sens, data, bool(flags))
                st, got, total = device_case(cs, data, flags)
                assert st == 0 and total == want[0].size
                ref.same(got, want, f"{name}/device/flags {flags}")
                if name in ref.WANT:
                    ids, pos = ref.WANT[name][flags]
                    ref.same(got, (pos, ids), f"{name}/device/flags {flags}: against the list worked out by hand")
                st, got, total = device_pairs(cs, address, n, flags, pair_ids, pair_pos, int(want[0].size) + 3)
                assert st == 0
                ref.same(got, want, f"{name}/pairs/flags {flags}")
                ref.same(cs.match_host_array(as_array(data), bool(flags)), want, f"{name}/host form/flags {flags}")      # the GPU platform: the pipelined pairs path
    finally:
        h.destroy()


# ---------------------------------------------------------------- alignment


@pytest.mark.parametrize("in_offset", [0, 1, 2, 3])
def test_input_pointer_off_alignment_and_a_match_as_the_last_bytes(in_offset):
    """the compare composes the input's dwords from aligned ones: with the pointer 1 - 3 bytes off, the aligned dword in front of in[0] and the one
    behind in[n - 1] must not be loaded whole.  The edge input has a candidate at every residue mod 4 and ends with a sensitive match; the bytes in
    front of in[0] are letters that would complete nothing"""
    pats, sens, data = ref.EDGE_PATS, [1] * len(ref.EDGE_PATS), ref.edge_input()
    # also a sensitive match at position 0: the first aligned dword of a misaligned buffer reaches in front of it
    data = ref.edge_pattern(5) + b" " + data
    n = len(data)
    h = gpu_handle(pats)
    try:
        with h.caseOpen(text_of(pats), ref.flags_by_id(sens)) as cs:
            d_in, address = device_input(data, in_offset)
            assert address % 4 == in_offset and d_in.numel() == in_offset + n, "the tensor ends with the input's last byte"
            pair_ids, pair_pos = longest_pairs(h, address, n)
            assert set(int(p) & 3 for p in pair_pos) == {0, 1, 2, 3} and int(pair_pos[0]) == 0
            for flags in (0, ALL):
                want = ref.case_brute(pats, sens, data, bool(flags))
                assert int(want[0][0]) == 0 and int(want[0][-1]) + 33 == n, "a match at in[0], a match as the last bytes"
                st, got, total = device_case(cs, data, flags, in_offset=in_offset)
                assert st == 0
                ref.same(got, want, f"offset {in_offset}/device/flags {flags}")
                st, got, total = device_pairs(cs, address, n, flags, pair_ids, pair_pos, n)
                assert st == 0
                ref.same(got, want, f"offset {in_offset}/pairs/flags {flags}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- pair counts around the block, more than one grid pass


@pytest.mark.parametrize("pairs", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_pair_counts_around_the_block(pairs):
    pats, sens = [b"aB", b"ab", b"A"], [1, 0, 1]
    rng = np.random.Generator(np.random.PCG64(pairs))
    data = b"".join((b"aB ", b"ab ", b"AB ", b"Ab ")[int(k)] for k in rng.integers(0, 4, pairs))
    h = gpu_handle(pats)
    try:
        with h.caseOpen(text_of(pats), ref.flags_by_id(sens)) as cs:
            d_in, address = device_input(data)
            assert longest_pairs(h, address, len(data))[0].size == pairs
            for flags in (0, ALL):
                want = ref.case_brute(pats, sens, data, bool(flags))
                st, got, total = device_case(cs, data, flags)
                assert st == 0 and total >= pairs
                ref.same(got, want, f"{pairs} pairs/flags {flags}")
    finally:
        h.destroy()


def test_more_pairs_than_one_grid_pass_takes():
    """one pair per byte, more of them than the frame's blocks take at one pair per thread: the blocks walk their pairs in several trips.  One
    letter in alternating case under the one-byte patterns `a` and `A`, both sensitive; list and ALL are the same list, worked out with numpy"""
    pats, sens = [b"a", b"A"], [1, 1]
    h = gpu_handle(pats)
    try:
        n = PER_CU * BLOCK * int(h.info().multiProcessorCount) + BLOCK + 1
        assert 400_000 < n < 4_000_000
        data = np.where(np.arange(n) % 2 == 0, ord("a"), ord("A")).astype(np.uint8)
        data[n // 3:n // 3 + 5] = ord("A")
        want_ids = torch.from_numpy(np.where(data == ord("a"), 1, 2).astype(np.int32)).to("cuda:0")
        want_pos = torch.arange(n, dtype=torch.int32, device="cuda:0")
        with h.caseOpen(text_of(pats), ref.flags_by_id(sens)) as cs:
            for flags in (0, ALL):
                st, (pos, ids), total = device_case(cs, data, flags, keep_on_device=True)
                assert (st, total) == (0, n)
                assert torch.equal(pos, want_pos) and torch.equal(ids, want_ids), f"flags {flags}"
    finally:
        h.destroy()


# ---------------------------------------------------------------- the pairs form


HOSTILE_PATS = [b"foo", b"fooBar", b"bar", b"O", b"foob", b"o", b"FOO"]          # (the folded set holds `foo` as id 7 and `o` as id 6)
HOSTILE_SENS = [0, 1, 0, 1, 1, 0, 1]


def test_pairs_form_ignores_what_lies_outside_the_set_and_the_buffer():
    pats, sens = HOSTILE_PATS, HOSTILE_SENS
    f = len(pats)
    data = b"foo bar fooBar FOO"
    n = len(data)
    h = gpu_handle(pats)
    try:
        with h.caseOpen(text_of(pats), ref.flags_by_id(sens)) as cs:
            d_in = torch.full((GUARD + n + GUARD,), ord("o"), dtype=torch.uint8, device="cuda:0")      # what a read outside the buffer would find
            d_in[GUARD:GUARD + n] = torch.from_numpy(as_array(data).copy())
            before = d_in.clone()
            address = d_in.data_ptr() + GUARD
            junk_ids = [0, -1, f + 1, 2**31 - 1, -2**31]
            junk_pos = [-1, -2**31, n, n + 1, 2**31 - 1]
            pair_ids = np.array([7, 2, 3, 2, 2, 7, 5, 4, 6, 1] + junk_ids + [7] * len(junk_pos) + [2, 2, 7, 6], dtype=np.int32)
            pair_pos = np.array([0, 0, 4, 8, 15, 15, 15, 1, 1, 8] + [8] * len(junk_ids) + junk_pos + [n - 5, n - 3, n - 2, n - 1], dtype=np.int32)
            for flags in (0, ALL):
                want = pairs_by_definition(pair_ids, pair_pos, pats, sens, data, bool(flags))
                st, got, total = device_pairs(cs, address, n, flags, pair_ids, pair_pos, 64)
                assert (st, total) == (0, want[0].size)
                ref.same(got, want, f"flags {flags}")
                # a capacity smaller than the total: exactly the first pairs, the full length
                st, got, t2 = device_pairs(cs, address, n, flags, pair_ids, pair_pos, total - 2)
                assert (st, t2) == (TRUNCATED, total)
                ref.same(got, (want[0][:total - 2], want[1][:total - 2]), f"flags {flags}/capacity {total - 2}")
                assert device_pairs(cs, address, n, flags, pair_ids, pair_pos, 0)[::2] == (TRUNCATED, total), "the count query"
                # an unsorted list: unspecified values, nothing outside the arrays (device_pairs checks the guards), no more pairs than the chains hold
                order = np.random.Generator(np.random.PCG64(3)).permutation(pair_ids.size)
                st, got, t3 = device_pairs(cs, address, n, flags, pair_ids[order], pair_pos[order], 64)
                assert st == 0 and t3 <= cs.max_matches_per_position * pair_ids.size
            # worked out by hand, ALL: a member that does not fit the buffer is not kept, its prefixes are
            got = device_pairs(cs, address, n, ALL, np.array([2, 2, 7, 6], dtype=np.int32), np.array([n - 5, n - 3, n - 2, n - 1], dtype=np.int32), 16)[1]
            assert got[0].tolist() == [n - 5, n - 3, n - 3, n - 1, n - 1] and got[1].tolist() == [1, 7, 1, 6, 4], \
                "fooBar never fits; `foob` fits at n - 5 but the bytes are `r FO`: only the caseless `foo` holds; FOO is there at n - 3; `o` and `O` at n - 1"
            assert torch.equal(d_in, before), "the caller's input, or what lies around it, was modified"
    finally:
        h.destroy()


def test_pairs_form_refuses_overlapping_arrays_and_takes_any_capacity():
    pats = [b"Ab", b"cd"]
    h = gpu_handle(pats)
    try:
        with h.caseOpen(text_of(pats), [0, 1, 0]) as cs:
            d_in = torch.from_numpy(as_array(b"Ab cd ab").copy()).to("cuda:0")
            buf = torch.full((64,), POISON, dtype=torch.int32, device="cuda:0")
            buf[0:3] = torch.tensor([1, 2, 1], dtype=torch.int32)
            buf[8:11] = torch.tensor([0, 3, 6], dtype=torch.int32)
            before = buf.clone()
            B = buf.data_ptr()
            call = lambda ids, pos, cap: cs.pairs_device(d_in.data_ptr(), 8, 0, B, B + 32, 3, ids, pos, cap, check=False)  # noqa: E731
            for ids, pos in ((B, B + 128), (B + 128, B + 32), (B + 8, B + 128), (B + 128, B + 40), (B + 36, B + 128)):
                assert call(ids, pos, 3)[0] == INVALID
            assert call(B + 4, B + 128, 2)[0] == INVALID and call(B + 12, B + 128, 1) == (TRUNCATED, 2), "arrays that touch but do not overlap"
            assert call(None, None, 0) == (TRUNCATED, 2), "the count query"
            torch.cuda.synchronize()
            assert torch.equal(buf[:3], before[:3]) and torch.equal(buf[8:11], before[8:11]) and torch.equal(buf[40:], before[40:])
            assert call(B + 128, B + 192, 16) == (0, 2)
            torch.cuda.synchronize()
            assert buf[32:34].tolist() == [1, 2] and buf[48:50].tolist() == [0, 3] and bool((buf[34:48] == POISON).all()) and bool((buf[50:] == POISON).all())
            # the match form: capacity >= size, and an unknown flag
            ids, pos = out_arrays(8)
            assert cs.match_device(d_in.data_ptr(), 8, 0, ids.data_ptr(), pos.data_ptr(), 7, check=False)[0] == INVALID
            assert cs.match_device(d_in.data_ptr(), 8, 2, ids.data_ptr(), pos.data_ptr(), 8, check=False)[0] == INVALID
    finally:
        h.destroy()


def test_tables_are_state_of_the_object_and_a_reread_makes_it_stale():
    pats, sens = HOSTILE_PATS, HOSTILE_SENS
    data = as_array(b"foo bar fooBar FOO o O" * 20)
    h = gpu_handle(pats)
    try:
        tables = h.info().deviceTableBytes
        cs = h.caseOpen(text_of(pats), ref.flags_by_id(sens))
        assert h.info().deviceTableBytes == tables, "nothing goes up before the first device call"
        want = ref.case_brute(pats, sens, data.tobytes(), True)
        ref.same(device_case(cs, data, ALL)[1], want, "the first device call")
        distinct = len(ref.distinct_patterns(pats, sens))
        blob = sum((len(p) + 3) // 4 * 4 for (s, p) in ref.distinct_patterns(pats, sens) if s)
        assert h.info().deviceTableBytes - tables == 8 * distinct + 4 * (len(pats) + 2) + blob, "8 bytes per distinct pattern, 4 (F + 2), the blob"
        scratch = h.info().deviceScratchBytes
        h.trim()
        assert h.info().deviceScratchBytes < scratch and h.info().deviceTableBytes - tables == 8 * distinct + 4 * (len(pats) + 2) + blob, "trim keeps the tables"
        ref.same(device_case(cs, data, ALL)[1], want, "the call works again after the trim")
        h.readPatternFromMemoryEx(text_of(pats), NOCASE)
        d_in, address = device_input(data)
        ids, pos = out_arrays(data.size)
        assert cs.match_device(address, data.size, 0, ids.data_ptr(), pos.data_ptr(), data.size, check=False)[0] == INVALID
        assert cs.pairs_device(address, data.size, 0, ids.data_ptr(), pos.data_ptr(), 2, None, None, 0, check=False)[0] == INVALID
        assert cs.close() == 0
        with h.caseOpen(text_of(pats), ref.flags_by_id(sens)) as fresh:
            ref.same(device_case(fresh, data, ALL)[1], want, "a new object on the new set")
    finally:
        h.destroy()


# ---------------------------------------------------------------- a seeded random set


def random_set(rng, lines=2000):
    """lines over the letters a - d: stems of 3 - 24 letters, many of them prefixes of others; every stem in up to five casings, each casing under a
    random flag, some twice"""
    stems = set()
    while len(stems) < lines // 4:
        stem = bytes(rng.choice(np.frombuffer(b"abcd", dtype=np.uint8), size=int(rng.integers(5, 25))))
        stems.add(stem)
        stems.add(stem[:int(rng.integers(3, len(stem) + 1))])
    stems = sorted(stems)
    pats, sens = [], []
    while len(pats) < lines:
        stem = stems[int(rng.integers(0, len(stems)))]
        flips = rng.random(len(stem)) < (0.0 if rng.random() < 0.3 else 0.4)
        pats.append(bytes(b ^ 0x20 if f else b for b, f in zip(stem, flips)))
        sens.append(int(rng.random() < 0.6))
    return pats, sens


def test_a_seeded_random_set_of_mixed_flags_over_a_mebibyte():
    rng = np.random.Generator(np.random.PCG64(20261020))
    pats, sens = random_set(rng)
    n = 1 << 20
    data = rng.choice(np.frombuffer(b"abcdABCD \n", dtype=np.uint8), size=n, p=[0.08] * 4 + [0.02] * 4 + [0.3, 0.3]).astype(np.uint8)
    for at in rng.integers(0, n - 32, 30000):                   # the lines themselves, a quarter of their letters flipped
        pat = np.frombuffer(pats[int(rng.integers(0, len(pats)))], dtype=np.uint8)
        data[at:at + pat.size] = np.where(rng.random(pat.size) < 0.25, pat ^ 0x20, pat)
    h = gpu_handle(pats)
    try:
        with h.caseOpen(text_of(pats), ref.flags_by_id(sens)) as cs:
            assert cs.max_matches_per_position == ref.max_per_position(pats, sens) > 3
            want_all = ref.case_brute(pats, sens, data.tobytes(), True)
            first = np.flatnonzero(np.concatenate(([True], want_all[0][1:] != want_all[0][:-1])))
            assert want_all[0].size > first.size + 10000 and first.size > 20000, "many positions with several patterns"
            for flags, want in ((0, (want_all[0][first], want_all[1][first])), (ALL, want_all)):
                st, got, total = device_case(cs, data, flags, capacity=max(n, int(want[0].size)))
                assert (st, total) == (0, want[0].size)
                ref.same(got, want, f"device/flags {flags}")
                ref.same(cs.match_host_array(data, bool(flags)), got, f"the host form against the device form/flags {flags}")
    finally:
        h.destroy()
