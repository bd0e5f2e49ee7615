"""Host bookkeeping of rolling-batch captioning (ImageToTextModel.generate_rolling_iter): which image sits in which
decode slot, which slots the last poll saw done, the next admission, the K/V pool and when the next encoder chunk is
due, and termination. Pure Python -- no torch, no GPU -- and driven only by (done flags, row_pos) snapshots, so the
whole schedule is testable on the CPU (tests/test_rolling_contract_cpu.py).

The pool is `pool` entries in regions of `encode_batch` entries; an encoder chunk fills one region, image j of the
chunk into entry region * encode_batch + j, and a region is free for the next chunk once every image of it that
needed a slot has been admitted (admission copies the entry's K/V into the slot). The loop of a driver:

    while True:
        while True:
            while sch.wants_chunk():
                chunk = next(source, None)
                if chunk is None: sch.close(); break
                at, trivial = sch.add_chunk(caps of the chunk)  # encode, K/V into pool entries at ..; trivial: cap 1
            triples = sch.admissions()                       # (slot, entry, cap): one admit launch, issued BEFORE
            if not (triples and sch.wants_chunk()): break    # the next chunk overwrites the region it reads from
        if sch.finished(): break
        run sch.next_steps() token steps
        sch.poll(done, row_pos) -> (slot, image, n_ids)      # newly done: copy their ids BEFORE the next admissions

samples = N > 1 (ImageToTextModel.generate_stream_iter): an image that needs a slot becomes N work items that share
its one pool entry; item n of image i has the row id i * N + n, takes its own slot (admissions_ex names the row id;
poll returns it in the place of the image) and the region is free once all the items of its images are admitted.
With samples = 1 an item is its image and nothing changes.
"""
from collections import deque
from typing import List, Optional, Sequence, Tuple

CHECK_EVERY_DEFAULT = 2  # of 1 / 2 / 4 / 8 the best median on the ragged benchmark (2 and 4 within each other's spread)


class RollingScheduler:
    def __init__(self, slots: int, check_every: Optional[int] = None, encode_batch: Optional[int] = None,
                 pool: Optional[int] = None, samples: int = 1):
        check_every = CHECK_EVERY_DEFAULT if check_every is None else int(check_every)
        encode_batch = slots if encode_batch is None else int(encode_batch)
        if slots < 1:
            raise ValueError(f"rolling decode needs slots >= 1 (got {slots})")
        if check_every < 1:
            raise ValueError(f"check_every must be at least 1 (got {check_every})")
        if encode_batch < 1:
            raise ValueError(f"encode_batch must be at least 1 (got {encode_batch})")
        if int(samples) < 1:
            raise ValueError(f"samples must be at least 1 (got {samples})")
        self.samples = int(samples)
        pool = max(slots, encode_batch) // encode_batch * encode_batch if pool is None else int(pool)
        if pool < encode_batch or pool % encode_batch:
            raise ValueError(f"the pool ({pool}) must be a positive multiple of encode_batch ({encode_batch})")
        self.slots, self.check_every, self.encode_batch, self.pool = slots, check_every, encode_batch, pool
        # the image a slot decodes (with samples > 1: the row id image * samples + n), None: empty / harvested
        self.slot_image: List[Optional[int]] = [None] * slots
        self.slot_cap = [0] * slots
        self.slot_pos = [0] * slots                            # row_pos of the slot at the last poll
        self.ready = deque()                                   # (item, pool entry, cap): K/V in the pool, no slot yet
        self.region_left = [0] * (pool // encode_batch)        # items of a region still waiting for a slot
        self.fill_region = 0
        self.next_image = 0
        self.exhausted = False
        self.steps = self.polls = self.admits = self.chunks = 0

    # --- the source ------------------------------------------------------------------------------------
    def free_slots(self) -> List[int]:
        return [s for s, im in enumerate(self.slot_image) if im is None]

    def wants_chunk(self) -> bool:
        """The pool runs low (no more images ready than free slots) and the next region is free."""
        return (not self.exhausted and self.region_left[self.fill_region] == 0
                and len(self.ready) <= len(self.free_slots()))

    def add_chunk(self, caps: Sequence[int]) -> Tuple[int, List[int]]:
        """The next len(caps) images of the source, with their caps (ids an image may have, >= 1). Returns (at,
        trivial): the chunk's K/V goes to pool entries at .. at + len(caps) - 1 (image j to entry at + j); the
        images of `trivial` have cap 1, are complete as [START] and take no slot."""
        n = len(caps)
        if not 1 <= n <= self.encode_batch:
            raise ValueError(f"a chunk holds 1..{self.encode_batch} images (got {n})")
        r = self.fill_region
        if self.exhausted or self.region_left[r]:
            raise RuntimeError("add_chunk without wants_chunk")
        for j, cap in enumerate(caps):
            if cap < 1:
                raise ValueError(f"image {self.next_image + j}: cap {cap} < 1")
        at, trivial = r * self.encode_batch, []
        for j, cap in enumerate(caps):
            if cap == 1:
                trivial.append(self.next_image + j)
            else:
                for n_ in range(self.samples):
                    self.ready.append(((self.next_image + j) * self.samples + n_, at + j, int(cap)))
                self.region_left[r] += self.samples
        self.next_image += n
        self.fill_region = (r + 1) % len(self.region_left)
        self.chunks += 1
        return at, trivial

    def close(self):
        """The source has no more images."""
        self.exhausted = True

    # --- slots -----------------------------------------------------------------------------------------
    def admissions(self) -> List[Tuple[int, int, int]]:
        """(slot, pool entry, cap) for every free slot that a ready image can take, in slot order; the slots are
        occupied from here on."""
        return [t[:3] for t in self.admissions_ex()]

    def admissions_ex(self) -> List[Tuple[int, int, int, int]]:
        """admissions() with the item admitted: (slot, pool entry, cap, row id = image * samples + n)."""
        out = []
        for s in self.free_slots():
            if not self.ready:
                break
            image, entry, cap = self.ready.popleft()
            self.slot_image[s], self.slot_cap[s], self.slot_pos[s] = image, cap, 0
            self.region_left[entry // self.encode_batch] -= 1
            out.append((s, entry, cap, image))
        if out:
            self.admits += 1
        return out

    def next_steps(self) -> int:
        """Token steps to run before the next poll: check_every, or fewer when no occupied slot can use that many
        (its cap leaves cap - 1 - row_pos steps); 0 with no occupied slot."""
        room = [self.slot_cap[s] - 1 - self.slot_pos[s] for s, im in enumerate(self.slot_image) if im is not None]
        n = min(self.check_every, max(room)) if room else 0
        self.steps += n
        return n

    def poll(self, done: Sequence[int], row_pos: Sequence[int]) -> List[Tuple[int, int, int]]:
        """A snapshot of the device's done flags and positions. Returns (slot, image, n_ids) for every occupied slot
        seen done: its caption is ids[slot, :n_ids], to be copied before the slot is reused; the slot is free. With
        samples > 1 `image` is the item's row id (image, n = divmod(row id, samples))."""
        self.polls += 1
        out = []
        for s, image in enumerate(self.slot_image):
            if image is None:
                continue
            self.slot_pos[s] = int(row_pos[s])
            if done[s]:
                out.append((s, image, int(row_pos[s]) + 1))
                self.slot_image[s] = None
        return out

    def finished(self) -> bool:
        """The source is exhausted, nothing waits in the pool and every slot is empty."""
        return self.exhausted and not self.ready and all(im is None for im in self.slot_image)
