"""The device-only chained table (PFACX_TABLE_CHAIN) walked in Python the way the filter kernel's walkers do (test infrastructure;
contract: struct ChainSlot in pfac_amd/csrc/pfac_context.h and the layout described in tables.cpp): first slot from the jump table at
hash(first four bytes), restart in the initial state's bucket if that slot is somebody else's, then one slot per transition with its
chain.  No prefilter: the tables alone must be exact."""
from pfac_amd import api

EMPTY, FINAL, WIDE = 1 << 14, 1 << 13, 1 << 15         # pfac_context.h: kSlotEmpty, kSlotFinal, kSlotWide; a leaf has k == 0
JUMP_MUL = 0x9E3779B1                                  # kJumpMul
CHAIN_MAX, CHAIN_MAX_WIDE = 7, 23                      # kChainMax, kChainMaxWide


def jump_hash(key32, log2_slots):
    return ((key32 * JUMP_MUL) & 0xFFFFFFFF) >> (32 - log2_slots)


class ChainWalker:
    """The chained table of a handle whose patterns are read.  Counters over everything walked so far:
      short_slot_steps slots looked at, matching or not, that fold at most 7 chain bytes (their extension unit is checked to be empty)
      long_slots       matching transitions through a slot that folds more than 7 chain bytes (bytes 8.. in its extension unit)
      chain_lengths    the chain lengths of the matching transitions met behind the first one of a walk
      fell_back        walks whose jump slot was somebody else's (or empty) and that restarted in the initial state's bucket
      bucket_sizes     the sizes S of the buckets that matching transitions led into
      mid_finals       matching transitions into a final state WITH successors (the id in chain[4..7]: the slot was cut early)"""

    def __init__(self, h):
        self.slots = h.table(api.PFACX_TABLE_CHAIN).reshape(-1, 4)
        self.info = info = h.info()
        self.J = J = info.chainJumpLog2
        assert 10 <= J <= 20 and info.chainSlots == len(self.slots) and len(self.slots) % 2 == 0
        self.ext_delta = len(self.slots) // 2          # N slot headers, then N extension units: the unit of slot i at N + i
        self.jump_base = self.ext_delta - (2 << J)     # the jump table; behind it the LONG jump table (same hash, chains of up to 23 bytes)
        self.root_row = self.jump_base - 256
        self.short_slot_steps = self.long_slots = self.fell_back = self.mid_finals = 0
        self.chain_lengths, self.bucket_sizes = set(), set()
        self.data = b""

    def jump_slot(self, key32, long_jump=False):
        return self.jump_base + (long_jump << self.J) + jump_hash(key32, self.J)

    def step(self, at, wide, b0, p):
        """transition through the slot at index `at` (wide: the slot that led here says its bucket may hold long slots) on edge
        byte b0 with the input behind it at p: (ok, leaf, match id or 0, end row, ks, bytes consumed)"""
        slots, data, ext_delta = self.slots, self.data, self.ext_delta
        slot = slots[at]
        meta = int(slot[0])
        ln = (meta >> 8) & 0x1F
        chain = int(slot[2]).to_bytes(4, "little") + int(slot[3]).to_bytes(4, "little")
        if ln > 7:                                 # only slots of wide buckets fold more than 7 bytes: 8 in the header, the rest in the unit
            assert wide and ln <= 23
            chain += b"".join(int(v).to_bytes(4, "little") for v in slots[at + ext_delta])
        else:
            assert not slots[at + ext_delta].any()     # the unit of a short slot is never written
            self.short_slot_steps += 1
        ok = (meta & (EMPTY | 0xFF)) == b0 and chain[:ln] == data[p:p + ln]
        leaf = (meta >> 16) & 0xFF == 0
        ident = 0
        if ok and meta & FINAL:
            ident = int(slot[1]) if leaf else int(slot[3])
        if ok:
            self.long_slots += ln > CHAIN_MAX
            self.mid_finals += bool(meta & FINAL) and not leaf
            if not leaf:
                self.bucket_sizes.add((meta >> 24) + 1)
        return ok, leaf, ident, int(slot[1]), meta, 1 + ln

    def walk_all(self, stream, expect, long_jump=False, what=()):
        """walks from every position of `stream` whose longest pattern cannot reach the padding; asserts the oracle's result `expect`
        at each; -> (walks that used their jump slot, walks that fell back)"""
        info, step = self.info, self.step
        n = len(stream)
        self.data = data = bytes(stream) + bytes(80)
        limit = max(n - info.maxPatternLen, 0)    # beyond it a walk would read the padding
        used_jump = fell_back = 0
        for i in range(limit):
            x = int.from_bytes(data[i:i + 4], "little")
            match = 0
            ok, leaf, ident, row, ks, used = step(self.jump_slot(x, long_jump), long_jump, data[i], i + 1)
            if ok:
                used_jump += 1
            else:                                  # restart in the initial state's bucket (k = 128, S = 256: the byte itself)
                fell_back += 1
                ok, leaf, ident, row, ks, used = step(self.root_row + data[i], False, data[i], i + 1)
            depth = 0
            while ok:
                if ident:
                    match = ident
                depth += used
                if leaf:
                    break
                b0 = data[i + depth]
                r = ((((ks >> 16) & 0xFF) * b0) >> 7) & (ks >> 24)        # pfac_context.h: chainSlotOf
                ok, leaf, ident, row, ks, used = step(row + r, bool(ks & WIDE), b0, i + depth + 1)   # only the slots of WIDE buckets may be long
                if ok:
                    self.chain_lengths.add(used - 1)
            assert match == int(expect[i]), (*what, i, match, int(expect[i]))
        self.fell_back += fell_back
        return used_jump, fell_back
