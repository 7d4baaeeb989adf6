"""What include/ibftgpu.h (ibft_cache_memory) and DESIGN.md promise about the slots of the per-device key cache, restated:
an address holds one slot while any referrer's current set (a context's, a family's) contains it; a slot nobody refers to
is free again and remembers nothing; a new address takes a slot while the pool is below the budget, in set order, and goes
without one otherwise; a table belongs to the address, so every referrer of the address sees it.  The model's slot numbers
are its own: only counts are compared with the library."""

SLOT_BYTES = 655360                 # one validator's table (32 windows × 256 entries × 80 B)
G_TABLE_BYTES = 16 * 65536 * 80     # the device's one fixed-base table of G (84 MB)


class KeyCacheModel:
    def __init__(self, budget_bytes=64 << 30):
        self.max_slots = budget_bytes // SLOT_BYTES
        self.slot = {}       # address → slot
        self.refs = {}       # slot → referrers
        self.built = set()   # addresses whose table is built
        self.sets = {}       # referrer → its current set's distinct addresses, in set order
        self._next = 0

    @property
    def slots_in_use(self):
        return len(self.slot)

    def _drop(self, who):
        for a in self.sets.pop(who, []):
            if a in self.slot:
                self.refs[self.slot[a]] -= 1
                if self.refs[self.slot[a]] == 0:
                    del self.refs[self.slot.pop(a)]
                    self.built.discard(a)

    def set_validators(self, who, addrs):
        """→ (indices, among the set's distinct addresses in set order, of validators WITHOUT a slot; tables `who` counts)"""
        new = list(dict.fromkeys(bytes(a) for a in addrs))
        for a in new:                                   # an address in both sets never drops to zero in between
            if a in self.slot:
                self.refs[self.slot[a]] += 1
        self._drop(who)
        for a in new:
            if a not in self.slot and len(self.slot) < self.max_slots:
                self.slot[a], self._next = self._next, self._next + 1
                self.refs[self.slot[a]] = 1
        self.sets[who] = [a for a in new if a in self.slot]
        return [i for i, a in enumerate(new) if a not in self.slot], self.tables(who)

    def close(self, who):
        self._drop(who)

    def learned(self, addrs):
        """a valid signature of each of these addresses was seen and the build pass behind it has run"""
        self.built.update(a for a in (bytes(x) for x in addrs) if a in self.slot)

    def tables(self, who):
        return sum(a in self.built for a in self.sets[who])

    def check_capacity(self, used, cap, device_bytes):
        """the growth factor is the allocator's choice: only the bounds are promised"""
        assert used == self.slots_in_use, (used, self.slots_in_use)
        assert used <= cap <= self.max_slots, (used, cap, self.max_slots)
        assert device_bytes <= G_TABLE_BYTES + (cap + 1) * 660000, (device_bytes, cap)
