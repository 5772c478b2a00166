"""A stand-in for the torch handle of one engine (`eng._torch = Guarded(torch, fill)`) that puts every output array the wrapper
allocates between two guards and fills the whole with one byte: tests/test_output_bounds_gpu.py asks afterwards whether a call
wrote outside an output (a stray write) and whether it left a word of an output as it found it (a stale word).  No tests here;
no library code changes and nothing is patched globally -- every attribute but `empty` is torch's own.

What `empty` hands out:

    | GUARD bytes of fill | nbytes of the output, filled | slack up to a multiple of 256, filled | GUARD bytes of fill |
                          ^ 256-byte aligned: the view the wrapper gets

THE REACH.  GUARD is 64 KiB on each side.  The widest row here is 64 x 4 B, so a stray block of 256 rows before or behind an
output lands inside the guard and is seen.  A write farther away than 64 KiB from the output it belongs to is out of this
helper's reach: it lands in some other allocation, as it would without the helper.

The questions are answered on the tensors' own device with a few torch reductions; the guards are never copied to the host.
"""
import linecache
import re
import sys

GUARD = 64 << 10
ALIGN = 256


def fill_word(fill):
    return fill * 0x01010101


class Record:
    """One allocation: `buffer` (uint8: guard, interior, slack, guard), `nbytes` of the interior that were asked for, `shape`,
    `dtype`, `method` -- the wrapper method that asked --, `name`, "<method>#<its ordinal among that method's>", and `spare`: whether
    the wrapper's source line assigns it to `spare`."""

    def __init__(self, name, buffer, nbytes, shape, dtype, method, view):
        self.name, self.buffer, self.nbytes, self.shape, self.dtype, self.method, self.view = name, buffer, nbytes, shape, dtype, method, view

    @property
    def interior(self):
        return self.buffer[GUARD:GUARD + self.nbytes]

    def __repr__(self):
        return "%s %s %s" % (self.name, tuple(self.shape), str(self.dtype).replace("torch.", ""))


class Guarded:
    def __init__(self, torch, fill):
        if not 0 <= int(fill) <= 255:
            raise ValueError("the fill is one byte")
        self._guarded_torch, self.fill, self.records = torch, int(fill), []

    def __getattr__(self, name):  # (only what the instance does not have itself: everything but `empty` and the helper's own)
        return getattr(self._guarded_torch, name)

    def empty(self, *size, dtype=None, device=None):
        torch = self._guarded_torch
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        shape = tuple(int(d) for d in shape)
        dtype = torch.get_default_dtype() if dtype is None else dtype
        count = 1
        for d in shape:
            count *= d
        nbytes = count * torch.empty((), dtype=dtype).element_size()
        rounded = -(-nbytes // ALIGN) * ALIGN
        raw = torch.full((GUARD + rounded + GUARD + ALIGN,), self.fill, dtype=torch.uint8, device=device)
        lead = -(raw.data_ptr() + GUARD) % ALIGN  # the allocator aligns to 512 B on the GPU, to 64 B on the host
        buffer = raw[lead:lead + GUARD + rounded + GUARD]
        view = buffer[GUARD:GUARD + nbytes].view(dtype).view(shape)
        frame = sys._getframe(1)
        method = frame.f_code.co_name
        name = "%s#%d" % (method, sum(r.method == method for r in self.records))
        record = Record(name, buffer, nbytes, shape, dtype, method, view)
        # the wrappers' `spare = torch.empty(...)`: the address a call is given for an EMPTY tensor, no output -- guarded, never written
        record.spare = re.match(r"\s*spare\s*=", linecache.getline(frame.f_code.co_filename, frame.f_lineno)) is not None
        self.records.append(record)
        return view

    # ---- the two questions ------------------------------------------------------------------------------------------------------------
    def by_name(self, name):
        for r in self.records:
            if r.name == name:
                return r
        raise KeyError(name)

    def name_of(self, tensor):
        """The record that `tensor` (an output, or a slice of one) lies in; None if the helper did not hand it out."""
        at = tensor.data_ptr()
        for r in self.records:
            lo = r.buffer.data_ptr() + GUARD
            if r.nbytes > 0 and lo <= at < lo + r.nbytes and tensor.device == r.buffer.device:
                return r.name
        return None

    def stray(self, limit=8):
        """[(record name, [offsets])]: the buffers with a guard byte, or a slack byte behind nbytes, that is no longer the fill, and
        the first `limit` such bytes as offsets relative to the interior (negative: in front of it; >= nbytes: behind it).  Call it
        once the stream has synchronised."""
        torch = self._guarded_torch
        if not self.records:
            return []
        counts = torch.stack([(r.buffer[:GUARD] != self.fill).sum() + (r.buffer[GUARD + r.nbytes:] != self.fill).sum() for r in self.records]).tolist()
        out = []
        for r, bad in zip(self.records, counts):
            if bad:
                front = torch.nonzero(r.buffer[:GUARD] != self.fill).reshape(-1) - GUARD
                behind = torch.nonzero(r.buffer[GUARD + r.nbytes:] != self.fill).reshape(-1) + r.nbytes
                out.append((r.name, torch.cat([front, behind])[:limit].tolist()))
        return out

    def as_filled(self, name, unit=4):
        """A boolean per `unit`-byte word of the output (4: a word; 1 for the byte-sized flags), on the buffer's device: whether the
        word still equals the fill word.  An output whose size is no multiple of the unit ends in a word that is part slack."""
        r = self.by_name(name)
        units = -(-r.nbytes // unit)
        return (r.buffer[GUARD:GUARD + units * unit].view(units, unit) == self.fill).all(dim=1)
