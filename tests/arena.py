"""Poisoned arenas: run an entry point on buffers the test owns on both sides and look at every byte it was not given.

Every buffer of a case gets an allocation of its own -- 1 MiB guard, payload, 1 MiB guard -- so an overrun of one buffer cannot hide in a neighbour.  1 MiB is
larger than any tile, LDS stage (160 KB) or DMA round of any kernel of the library; that is the only reason for the figure.  The payload starts at a 256-byte
boundary plus ``align``, the smallest alignment include/vd3d.h demands for that pointer (16 for ``X`` and the images, 4 where the header says 4-byte): every pointer
has exactly the demanded alignment and no more, which also runs the 4-byte load and store forms.

Guards, outputs and scratch are filled bytewise with each of ``FILLS``:
  0x00  the benign baseline;
  0xFF  NaN as float32 / bf16 / fp16, 255 as uint8, -1 as an integer;
  0x47  51015.28 as float32, about 51000 as bf16, about 7.28 as fp16, 71 as uint8: finite, positive and large beside the operands, so it shows a read that a NaN
        poison loses in a max, a min, a clamp or a compare-select.

Roles: ``input`` (payload = the operand; guards and payload bytewise unchanged afterwards), ``output`` (payload pre-filled with the fill), ``scratch`` (a weight
image or a workspace of exactly the entry point's own ``*_weight_bytes`` / ``*_workspace_bytes``, pre-filled with the fill; the back guard starts at that byte count;
``whole=True`` where every byte of it has to be defined by the call, as for a weight image).

``check_case`` asserts, naming the entry point, the buffer and the byte offset (from the payload's first byte; negative in the front guard) of the first differing byte:
  1. every guard of every buffer equals its fill under every fill;         2. every input payload is unchanged;
  3. outputs (and ``whole`` scratch) are bit-identical under the fills;      4. and bit-identical to what the ``Renderer`` wrapper returns in ordinary placement;
  5. float outputs are finite (the operands are);                           6. the return code is 0;
and, where the case gives one, that the outputs EQUAL an independent float64 result (exact-integer operands).

What it cannot see: a read outside a buffer whose value is then discarded, and any access more than 1 MiB away from the payload.  Nothing here places a buffer
against the end of an allocation or tries to make a kernel fault: an overrun shows as a changed guard byte.

The module works on CPU tensors too (tests/test_arena_host.py runs NumPy "kernels" on CPU arenas), so the harness itself is tested without a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

GUARD = 1 << 20
FILLS = (0x00, 0xFF, 0x47)


class Arena:
    """One allocation: GUARD bytes, payload of ``nbytes`` at (256-byte boundary + ``align``), GUARD bytes, all ``fill``."""

    def __init__(self, nbytes: int, align: int = 16, fill: int = 0, device="cpu"):
        assert 0 < align < 256 and nbytes >= 0
        self.nbytes, self.align, self.fill = int(nbytes), int(align), int(fill)
        self.mem = torch.full((GUARD + 512 + self.nbytes + GUARD,), self.fill, dtype=torch.uint8, device=device)
        self.off = GUARD + (align - (self.mem.data_ptr() + GUARD)) % 256
        self.ptr = self.mem.data_ptr() + self.off
        assert self.ptr % 256 == align and self.off >= GUARD and self.off + self.nbytes + GUARD <= self.mem.numel()

    @property
    def payload(self) -> torch.Tensor:
        return self.mem[self.off:self.off + self.nbytes]

    def load(self, data: np.ndarray):
        b = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        assert b.size == self.nbytes
        self.payload.copy_(torch.from_numpy(b.copy()))

    def read(self) -> np.ndarray:
        return self.payload.cpu().numpy().copy()

    def guard_diff(self):
        """Payload-relative offset of the first guard byte (front first) that is not the fill, or None."""
        front, back = self.mem[:self.off], self.mem[self.off + self.nbytes:]
        for g, base in ((front, -self.off), (back, self.nbytes)):
            bad = g != self.fill
            if bool(bad.any()):
                return base + int(torch.nonzero(bad)[0, 0])
        return None


@dataclass
class Buf:
    name: str
    role: str                      # "input" | "output" | "scratch"
    align: int = 16
    data: np.ndarray | None = None  # input: the operand
    nbytes: int = 0                # output / scratch
    dtype: str | None = None       # output: NumPy dtype name of its elements ("float32", "uint8", ...; bf16 as "bfloat16")
    whole: bool = False            # scratch: every byte is defined by the call

    def size(self) -> int:
        return int(np.ascontiguousarray(self.data).nbytes) if self.role == "input" else int(self.nbytes)


@dataclass
class Case:
    entry: str                     # the entry point(s), as in include/vd3d.h
    shape: str                     # for the report line
    bufs: list
    call: object                   # call(env) -> return code; env.p[name] = address, env.a[name] = Arena
    wrapper: object = None         # wrapper(R, t) -> {output name: tensor in the raw call's memory order}; t[name] = the operand on the device
    exact: dict = field(default_factory=dict)   # {output name: expected array (from float64)}


@dataclass
class Env:
    p: dict
    a: dict
    device: object
    L: object = None
    ctx: object = None


@dataclass
class Run:
    fill: int
    rc: int
    outputs: dict                  # {name: uint8 array}
    problems: list                 # messages of assertions 1, 2 and 6


def _first_diff(a: np.ndarray, b: np.ndarray):
    if a.size != b.size:
        return min(a.size, b.size)
    d = np.flatnonzero(a != b)
    return int(d[0]) if d.size else None


def run_case(case: Case, fill: int, device="cpu", R=None) -> Run:
    """Build the arenas under ``fill``, run the case's call with pointers into them, synchronise once; outputs (and ``whole`` scratch) come back as byte arrays."""
    arenas = {}
    for b in case.bufs:
        a = arenas[b.name] = Arena(b.size(), b.align, fill, device)
        if b.role == "input":
            a.load(b.data)
    env = Env({n: a.ptr for n, a in arenas.items()}, arenas, device, getattr(R, "_L", None), getattr(R, "_ctx", None))
    if R is not None:
        R._enter()
    rc = int(case.call(env))
    if R is not None:
        torch.cuda.synchronize()
    problems, outputs = [], {}
    if rc != 0:
        problems.append(f"{case.entry} {case.shape}: return code {rc} under fill 0x{fill:02X}")
    for b in case.bufs:
        a = arenas[b.name]
        g = a.guard_diff()
        if g is not None:
            where = "front guard" if g < 0 else "back guard"
            problems.append(f"{case.entry} {case.shape}: buffer '{b.name}' ({b.role}): {where} changed under fill 0x{fill:02X}, first at byte offset {g} "
                            f"(payload is [0, {a.nbytes}))")
        if b.role == "input":
            d = _first_diff(a.read(), np.ascontiguousarray(b.data).reshape(-1).view(np.uint8))
            if d is not None:
                problems.append(f"{case.entry} {case.shape}: buffer '{b.name}' (input) was written under fill 0x{fill:02X}, first at byte offset {d}")
        elif b.role == "output" or b.whole:
            outputs[b.name] = a.read()
    return Run(fill, rc, outputs, problems)


def _as_float(raw: np.ndarray, dtype: str):
    if dtype == "bfloat16":
        return (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    dt = np.dtype(dtype)
    return raw.view(dt) if dt.kind == "f" else None


def check_case(case: Case, device="cpu", R=None, fills=FILLS) -> str:
    """The assertions of the module docstring; returns the report line ``ARENA <entry point> <shape> fills=N guards=ok bits=same exact=<yes|n/a>``."""
    runs = [run_case(case, f, device, R) for f in fills]
    problems = [m for r in runs for m in r.problems]
    assert not problems, "\n".join(problems)
    base = runs[0]
    for r in runs[1:]:
        for name, got in r.outputs.items():
            d = _first_diff(base.outputs[name], got)
            assert d is None, (f"{case.entry} {case.shape}: buffer '{name}' depends on memory the call did not write: fill 0x{base.fill:02X} and fill 0x{r.fill:02X} "
                               f"differ, first at byte offset {d}")
    dtypes = {b.name: b.dtype for b in case.bufs if b.role == "output"}
    for name, dt in dtypes.items():
        v = _as_float(base.outputs[name], dt) if dt else None
        if v is not None:
            bad = np.flatnonzero(~np.isfinite(v))
            assert bad.size == 0, f"{case.entry} {case.shape}: buffer '{name}': non-finite output, first at byte offset {int(bad[0]) * (v.itemsize if dt != 'bfloat16' else 2)}"
    if case.wrapper is not None and R is not None:
        t = {b.name: torch.from_numpy(np.ascontiguousarray(b.data)).to(device) for b in case.bufs if b.role == "input"}
        ref = case.wrapper(R, t)
        torch.cuda.synchronize()
        for name, tens in ref.items():
            want = tens.contiguous().cpu().reshape(-1).view(torch.uint8).numpy()
            d = _first_diff(base.outputs[name], want)
            assert d is None, f"{case.entry} {case.shape}: buffer '{name}' differs from the Renderer wrapper's result in ordinary placement, first at byte offset {d}"
    for name, exp in case.exact.items():
        dt = dtypes[name]
        got = _as_float(base.outputs[name], dt) if dt in ("float32", "bfloat16", "float16", "float64") else base.outputs[name].view(np.dtype(dt))
        exp = np.asarray(exp).reshape(-1)
        assert got.size == exp.size, f"{case.entry} {case.shape}: buffer '{name}': {got.size} elements, the float64 result has {exp.size}"
        bad = np.flatnonzero(got.astype(np.float64) != exp.astype(np.float64))
        assert bad.size == 0, (f"{case.entry} {case.shape}: buffer '{name}' is not the float64 result: first at byte offset {int(bad[0]) * (2 if dt == 'bfloat16' else got.itemsize)}: "
                               f"{got[bad[0]]!r} != {exp[bad[0]]!r} ({bad.size} elements)")
    line = f"ARENA {case.entry} {case.shape} fills={len(fills)} guards=ok bits=same exact={'yes' if case.exact else 'n/a'}"
    print(line)
    return line
