"""The recorder accumulators of a launch: where they lie (`TallyLayout`) and the device buffers that hold them (`TallySet`).

One int64 buffer holds, per tally set, `distinct[pad] | crossings[pad] | bins[n_bins] | map slots[map_slots]` (`pad` =
max(recorders, 1); the tail is at least one word) and one float64 buffer holds the moment sums `[pad, 4, 2]`; with
`PvtTraceParams.tally_bundle` both repeat once per set, `stride_i64` / `stride_f64` apart.  A scene with captured
recorders adds `capture_rows` rows of 96 bytes and one cursor per recorder, per set.  This module is the only place that
knows these offsets; `tally.py` is the host referee and has nothing to do with them.
"""
import ctypes as C

from pvtrace_amd.engine import native
from pvtrace_amd.engine.recorder import MAX_CAPTURE_ROWS, CapturedRays


class TallyLayout:
    """The numbers of one tally set of a compiled scene (no torch, no GPU)."""

    def __init__(self, compiled):
        self.n_rec = int(compiled.rec_node.shape[0])
        self.pad = max(self.n_rec, 1)
        self.n_bins = int(compiled.total_bins)
        self.map_slots = int(getattr(compiled, "map_slots", 0))   # (the volume maps' slots follow the bins)
        self.stride_i64 = 2 * self.pad + max(self.n_bins + self.map_slots, 1)
        self.stride_f64 = self.pad * 8
        self.capture_rows = int(getattr(compiled, "capture_rows", 0))

    def split(self, ints, sums):
        """One set's slice of the two buffers (numpy arrays or torch tensors) -> the reference's rec_* arrays, and
        `map_bins` when the scene has volume maps: views, nothing is copied."""
        r, bins = self.n_rec, 2 * self.pad
        maps = bins + self.n_bins
        out = {"rec_distinct": ints[:r], "rec_crossings": ints[self.pad:self.pad + r], "rec_bins": ints[bins:maps]}
        if self.map_slots:
            out["map_bins"] = ints[maps:maps + self.map_slots]
        out["rec_sums"] = sums[: r * 8].reshape(r, 4, 2)
        return out

    def struct(self, ints_address, sums_address):
        """PvtTallies over the two buffers at these (host or device) addresses."""
        return native.PvtTallies(native.addr_ptr(ints_address, C.c_int64),
                                 native.addr_ptr(ints_address + 8 * self.pad, C.c_int64),
                                 native.addr_ptr(sums_address, C.c_double),
                                 native.addr_ptr(ints_address + 16 * self.pad, C.c_int64))


class TallySet:
    """`sets` consecutive zeroed tally sets of a scene in two torch buffers (`ints`, `sums`), so that all of them are
    zeroed by two fills and all-reduced by two collectives.  A scene with captured recorders gets `cap_rows` (`sets` x
    `capture_rows` rows, up to 1.5 GiB per set, uninitialised: only rows below a cursor are ever read) and `cap_cursor`
    as well, unless `captures=False`: a buffer that no launch will append to; a launch given one keeps no rows."""

    def __init__(self, compiled, device, sets=1, captures=True):
        import torch

        self.layout = layout = TallyLayout(compiled)
        self.sets = int(sets)
        rows = layout.capture_rows if captures else 0
        if self.sets * rows > MAX_CAPTURE_ROWS:
            raise ValueError(f"{sets} tally sets of {rows} capture rows each exceed the {MAX_CAPTURE_ROWS} rows one buffer "
                             f"may hold; lower the recorders' `capture` or trace fewer bundles per launch")
        self.ints = torch.zeros(self.sets * layout.stride_i64, dtype=torch.int64, device=device)
        self.sums = torch.zeros(self.sets * layout.stride_f64, dtype=torch.float64, device=device)
        self.cap_rows = self.cap_cursor = None
        if rows:
            self.cap_rows = torch.empty((self.sets * rows, native.CAPTURE_ROW_WORDS), dtype=torch.int64, device=device)
            self.cap_cursor = torch.zeros(self.sets * layout.pad, dtype=torch.int64, device=device)
        # what `DeviceScene.trace` hands to the library
        self.struct = layout.struct(self.ints.data_ptr(), self.sums.data_ptr())
        self.capture_struct = None
        if rows:
            self.capture_struct = native.PvtCaptures(native.addr_ptr(self.cap_rows.data_ptr(), C.c_uint64),
                                                     native.addr_ptr(self.cap_cursor.data_ptr(), C.c_int64))

    def zero_(self, tallies=True, captures=True):
        """Zero the tallies (two fills) and forget the captured rows (one more, when there are any), on the current stream."""
        if tallies:
            self.ints.zero_()
            self.sums.zero_()
        if captures and self.cap_cursor is not None:
            self.cap_cursor.zero_()

    def add_(self, other):
        self.ints += other.ints
        self.sums += other.sums

    def all_reduce(self, group=None):
        """Sum the tallies over the ranks, in place (two collectives; captured rows stay on their rank)."""
        import torch.distributed as dist

        dist.all_reduce(self.ints, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.sums, op=dist.ReduceOp.SUM, group=group)

    def host(self, set_index=None, sets=None):
        """The tallies as host numpy arrays (`TallyLayout.split`): of set `set_index`, or a list for the first `sets`
        sets (default: all).  One device-to-host copy of each buffer, of the sets asked for only."""
        si, sf = self.layout.stride_i64, self.layout.stride_f64
        first, count = (0, self.sets if sets is None else sets) if set_index is None else (set_index, 1)
        ints = self.ints[first * si:(first + count) * si].cpu().numpy()
        sums = self.sums[first * sf:(first + count) * sf].cpu().numpy()
        parts = [self.layout.split(ints[j * si:(j + 1) * si], sums[j * sf:(j + 1) * sf]) for j in range(count)]
        return parts if set_index is None else parts[0]

    def captures(self, compiled, set_index=0, index_shift=0):
        """{recorder name: CapturedRays} of one set.  Per captured recorder the min(cursor, capacity) rows that were
        written are sorted by ray index on the GPU and only they are moved to the host.  `index_shift` is added to the
        indices (bundles of a stream that were traced with the stream position folded into the seed instead of the ray
        offset)."""
        if not self.layout.capture_rows:
            return {}
        import torch

        from pvtrace_amd.engine.api import to_host

        pad = self.layout.pad
        cursors = self.cap_cursor[set_index * pad:(set_index + 1) * pad].cpu().numpy()
        out = {}
        for r, spec in enumerate(compiled.recorder_specs):
            capacity = int(compiled.rec_capture_capacity[r])
            if capacity == 0:
                continue
            matched = int(cursors[r])
            n = min(matched, capacity)
            first = set_index * self.layout.capture_rows + int(compiled.rec_capture_start[r])
            block = self.cap_rows[first:first + n]
            if n > 1:
                block = block.index_select(0, torch.argsort(block[:, 0]))
            out[spec.name] = CapturedRays.from_rows(spec.name, capacity, matched, to_host(block.contiguous()), index_shift)
        return out
