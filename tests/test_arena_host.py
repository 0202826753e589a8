"""tests/arena.py must catch what it claims to: NumPy "kernels" on CPU arenas, one well-behaved and eight faulty in one way each, through ``check_case``.
No GPU.  The operation is y[i] = max(x) + ws[i] with ws[i] = 2 x[i] staged through a scratch buffer of N floats: small enough to state every fault in one line."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arena   # noqa: E402

N = 37
POKE = np.frombuffer(bytes([0x11] * 4), np.float32)[0]   # no byte of it is a fill byte or a byte of an operand


def _f32(env, name):
    """(the whole allocation as float32 counted from the payload's first byte, index of that byte's element): index -1 and N are guard elements."""
    a = env.a[name]
    raw = a.mem.numpy()
    lo = a.off % 4
    v = raw[lo:lo + (raw.size - lo) // 4 * 4].view(np.float32)
    return v, (a.off - lo) // 4


def _kernel(fault):
    def call(env):
        x, x0 = _f32(env, "x")
        y, y0 = _f32(env, "y")
        ws, w0 = _f32(env, "ws")
        xin = x[x0:x0 + N].copy()
        m = np.fmax.reduce(x[x0:x0 + N + (1 if fault == "e" else 0)])
        if fault == "d":
            m = np.float32(m + x[x0 + N])
        if fault != "g":
            ws[w0:w0 + N] = 2 * xin
        out = m + ws[w0:w0 + N]
        if fault == "g":
            ws[w0:w0 + N] = 2 * xin
        n = N - 1 if fault == "f" else N
        y[y0:y0 + n] = out[:n]
        if fault == "b":
            y[y0 + N] = POKE
        if fault == "c":
            y[y0 - 1] = POKE
        if fault == "h":
            x[x0 + 3] = POKE
        if fault == "i":
            env.a["ws"].mem.numpy()[env.a["ws"].off + 4 * N] = 1
        return 0
    return call


def _case(fault):
    x = (np.arange(N) % 13 + 1).astype(np.float32)   # positive, so the maximum is an operand and not a 0x00 guard
    return arena.Case(f"fake_{fault}", f"N={N}", [arena.Buf("x", "input", 16, data=x), arena.Buf("y", "output", 4, nbytes=4 * N, dtype="float32"),
                                                   arena.Buf("ws", "scratch", 16, nbytes=4 * N)], _kernel(fault),
                      exact={"y": 13.0 + 2.0 * x.astype(np.float64)})


def test_arena_layout():
    for align in (4, 16):
        for fill in arena.FILLS:
            a = arena.Arena(4 * N, align, fill)
            assert a.ptr % 256 == align and a.off >= arena.GUARD and a.mem.numel() - a.off - a.nbytes >= arena.GUARD
            assert a.guard_diff() is None and bool((a.payload == fill).all())
            a.mem[a.off - 1] = fill ^ 1
            assert a.guard_diff() == -1
            a.mem[a.off - 1] = fill
            a.mem[a.off + a.nbytes] = fill ^ 1
            assert a.guard_diff() == a.nbytes
    assert np.frombuffer(bytes([0x47] * 4), np.float32)[0] == np.float32(51015.27734375)
    assert np.isnan(np.frombuffer(bytes([0xFF] * 4), np.float32)[0]) and np.isnan(np.frombuffer(bytes([0xFF] * 2), np.float16)[0])
    assert abs(float(np.frombuffer(bytes([0x47] * 2), np.float16)[0]) - 7.28) < 0.01


def test_well_behaved_kernel_passes(capsys):
    line = arena.check_case(_case("a"))
    assert line == f"ARENA fake_a N={N} fills=3 guards=ok bits=same exact=yes" and line in capsys.readouterr().out


@pytest.mark.parametrize("fault,buf,offset,what", [
    ("b", "y", 4 * N, "back guard changed"),          # one element past the output
    ("c", "y", -4, "front guard changed"),            # one element before the output
    ("d", "y", 0, "depends on memory"),               # the element past the input added into a sum: every output moves with the fill
    ("f", "y", 4 * (N - 1), "depends on memory"),     # the last output element left unwritten
    ("g", "y", 0, "depends on memory"),               # scratch read before it is written
    ("h", "x", 4 * 3, "was written"),                 # a write into an input
    ("i", "ws", 4 * N, "back guard changed"),         # one byte past the scratch's byte count
])
def test_faulty_kernel_is_caught(fault, buf, offset, what):
    with pytest.raises(AssertionError) as e:
        arena.check_case(_case(fault))
    msg = str(e.value)
    assert f"fake_{fault}" in msg and f"buffer '{buf}'" in msg and what in msg, msg
    assert int(re.search(r"first at byte offset (-?\d+)", msg).group(1)) == offset, msg


def test_max_over_one_element_too_many_needs_the_finite_poison():
    """(e): np.fmax over a range one element too long.  fmax drops the NaN of 0xFF and the 0.0 of 0x00 is below every operand: those two fills agree and equal the
    float64 result.  Only 0x47 (51015.28) wins the maximum -- the reason the third fill exists."""
    case = _case("e")
    assert arena.check_case(case, fills=(0x00, 0xFF)).endswith("fills=2 guards=ok bits=same exact=yes")
    with pytest.raises(AssertionError) as e:
        arena.check_case(case)
    msg = str(e.value)
    assert "fake_e" in msg and "buffer 'y'" in msg and "fill 0x47" in msg and "fill 0xFF" not in msg and "first at byte offset 0" in msg, msg
