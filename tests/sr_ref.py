"""The definition of the stochastically rounded steps (include/pimemb_grad.h, THE STOCHASTICALLY ROUNDED STEPS) as a loop: the reference
of tests/test_sr_cpu.py and tests/test_gpu_grad_sr.py.
  philox4x32_10   Philox4x32-10 on numpy uint64 arithmetic (one block per entry of its arrays)
  enc_sr_value    enc_sr_T(x, R) by its definition on VALUES, one element, Python integers: lo, hi, f, F = floor(f * 2^32), the carry
  enc_sr          the same on arrays, by the header's recipe on the bits (tests/test_sr_cpu.py holds the two against each other)
  step            one step of a table: the sparse gradient of grad_ref (position order) or grad_seg_ref (segmented order), the fp32
                  arithmetic of grad_ref / optim_ref up to the value x, then enc_sr with the words of (seed, t, row, element)
Nothing here runs the code under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402
import grad_seg_ref as gs  # noqa: E402
import optim_ref as orf  # noqa: E402

F = np.float32
U64 = np.uint64
M32 = (1 << 32) - 1
KNOWN_ANSWERS = (      # (counter, key, output)
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((M32,) * 4, (M32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays: the output words of the blocks with counters (c0, c1, c2, c3) and key (k0, k1) (arrays or ints)."""
    c = [np.atleast_1d(np.asarray(v, dtype=U64)) & U64(M32) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & M32, int(k1) & M32
    for _ in range(10):
        p0 = U64(0xD2511F53) * c[0]
        p1 = U64(0xCD9E8D57) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ U64(k0), p1 & U64(M32), (p0 >> U64(32)) ^ c[3] ^ U64(k1), p0 & U64(M32)]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [v.astype(np.uint32) for v in c]


def words(seed, t, row, dim):
    """uint32 [dim]: R of elements 0 .. dim - 1 of `row` at step number t -- counter (row, d div 4, t_lo, t_hi), word d mod 4."""
    seed, t = int(seed) % (1 << 64), int(t) % (1 << 64)
    pieces = (dim + 3) // 4
    out = philox4x32_10(int(row), np.arange(pieces), t & M32, t >> 32, seed & M32, seed >> 32)
    return np.stack(out, axis=1).reshape(-1)[:dim]


def _enc_nearest(kind, bits32):
    x = np.array([bits32], dtype=np.uint32).view(F)
    return int(gr.encode(kind, x[None, :]).view(np.uint16)[0, 0])


def enc_sr_value(kind, bits32, R):
    """enc_sr_T of ONE fp32 pattern by the definition on values.  |x| = m * 2^(e' - 150) with the 24-bit significand m; T's grid
    around |x| has a spacing of 2^k such units (bf16: 16; fp16: 13 from 2^-14 up, else whatever makes it 2^-24)."""
    bits32, R = int(bits32), int(R)
    sign, a = bits32 >> 31, bits32 & 0x7FFFFFFF
    if a >= 0x7F800000:
        return _enc_nearest(kind, bits32)
    e = a >> 23
    e1 = max(e, 1)
    m = (a & 0x7FFFFF) | (0x800000 if e else 0)
    if kind == "f16" and a >= 0x47800000:                 # |x| >= 65536
        return 0x7C00 | (sign << 15)
    k = 16 if kind == "bf16" else (13 if e >= 113 else 126 - e1)
    lo = m >> k                                           # grid steps below |x|: truncation toward zero
    rem = m - (lo << k)
    Fr = (rem << 32) >> k                                 # floor(f * 2^32), f = rem / 2^k
    up = 1 if Fr + R >= (1 << 32) else 0
    mag = float(lo + up) * 2.0 ** (k + e1 - 150)          # lo or hi: representable in T, or the power of two that stands for inf
    val = np.array([-mag if sign else mag], dtype=np.float64)
    with np.errstate(over="ignore"):
        if kind == "bf16":
            out = int(val.astype(F).view(np.uint32)[0]) >> 16      # (exact: a bf16 value, or 2^128 -> inf)
        else:
            out = int(val.astype(np.float16).view(np.uint16)[0])   # (exact: an fp16 value, or 65536 -> inf)
    return out | (sign << 15)                             # (-0 stays -0)


def enc_sr(kind, x, R):
    """uint16 array: enc_sr_T of the float32 array x with the uint32 words R, by the recipe on the bits."""
    x = np.ascontiguousarray(x, dtype=F)
    u = x.view(np.uint32).astype(U64)
    R = np.asarray(R, dtype=np.uint32).astype(U64).reshape(x.shape)
    a = u & U64(0x7FFFFFFF)
    carry = lambda Fr: (Fr + R) >> U64(32)  # noqa: E731
    if kind == "bf16":
        out = (u >> U64(16)) + carry((u & U64(0xFFFF)) << U64(16))
    elif kind == "f16":
        sign = (u >> U64(16)) & U64(0x8000)
        e = a >> U64(23)
        up = a + (carry((a & U64(0x1FFF)) << U64(19)) << U64(13))
        normal = ((np.maximum(up, U64(0x38000000)) - U64(0x38000000)) >> U64(13)) | sign
        m = (a & U64(0x7FFFFF)) | np.where(e > 0, U64(0x800000), U64(0))
        s = U64(126) - np.maximum(e, U64(1))              # (meaningful below 2^-14 only: 14 .. 125)
        s = np.where(e >= 113, U64(14), s)
        lo = np.where(s >= 24, U64(0), m >> np.minimum(s, U64(24)))
        rem = np.where(s >= 24, m, m & ((U64(1) << np.minimum(s, U64(24))) - U64(1)))
        Fr = np.where(s <= 32, rem << (U64(32) - np.minimum(s, U64(32))), np.where(s >= 56, U64(0), rem >> np.clip(s, U64(32), U64(63)) - U64(32)))
        small = (lo + carry(Fr)) | sign
        out = np.where(e >= 113, normal, small)
        out = np.where(a >= U64(0x47800000), U64(0x7C00) | sign, out)
    else:
        raise ValueError(kind)
    nearest = gr.encode(kind, x.reshape(1, -1)).view(np.uint16).reshape(x.shape).astype(U64)
    return np.where(a >= U64(0x7F800000), nearest, out).astype(np.uint16)


def initial_state(optimizer, n, dim):
    return None if optimizer == "sgd" else np.zeros((n, dim) if optimizer == "adagrad" else (n,), F)


def step_rows(kind, table_bytes, state, rows, grads, optimizer, lr, eps, seed, t):
    """(table bytes, state) after the step of the rows `rows` with the row gradients `grads`: the loop over U."""
    table = np.array(table_bytes, copy=True)
    state = None if state is None else np.array(state, dtype=F, copy=True)
    dim = table.shape[1] // 2
    for k, r in enumerate(rows):
        r = int(r)
        w = gr.decode(kind, table[r][None, :])[0]
        g = np.asarray(grads[k], F)
        if optimizer == "sgd":
            with np.errstate(over="ignore", invalid="ignore", under="ignore"):
                prod = F(lr) * g
                x = w - prod
        elif optimizer == "adagrad":
            x, state[r] = orf.adagrad_values(w, g, state[r], lr, eps)
        elif optimizer == "rowwise":
            x, state[r] = orf.rowwise_values(w, g, state[r], lr, eps)
        else:
            raise ValueError(optimizer)
        table[r] = enc_sr(kind, x, words(seed, t, r, dim)).view(np.uint8)
    return table, state


def step(kind, table_bytes, state, ids, off, G, mode="sum", w=None, pad=None, optimizer="sgd", lr=0.1, eps=1e-10, seed=0, t=0, segment=None):
    """One stochastically rounded step of one table: (table bytes, state, rows of U, number of bad positions)."""
    n = table_bytes.shape[0]
    if segment is None:
        rows, g, n_bad = gr.sparse_grad(n, ids, off, G, mode, w, pad)
    else:
        rows, g, n_bad = gs.seg_sparse_grad(n, ids, off, G, segment, mode, w, pad)
    table, state = step_rows(kind, table_bytes, state, rows, g, optimizer, lr, eps, seed, t)
    return table, state, rows, n_bad


# ---- the drift case: what stochastic rounding is for ------------------------------------------------------------------------------------
DRIFT_ROWS, DRIFT_DIM, DRIFT_STEPS = 32, 128, 64
DRIFT_LR = 2.0 ** -12
DRIFT_SEED = 0x5EED0123456789AB
DRIFT_ULPS = 8266            # the total the definition gives for this seed; expectation 8192, standard deviation 89


def drift_batch():
    """(ids, offsets, G): one-index bags that name every row once, G = -1."""
    ids = list(range(DRIFT_ROWS))
    return ids, np.arange(DRIFT_ROWS, dtype=np.int64), np.full((DRIFT_ROWS, DRIFT_DIM), -1.0, F)


def drift_table():
    return gr.encode("bf16", np.ones((DRIFT_ROWS, DRIFT_DIM), F))


def drift_tables(stochastic=True):
    """The table after every step t = 0 .. 63 of the drift case (stochastic=False: the plain in-place step)."""
    ids, off, G = drift_batch()
    table, out = drift_table(), []
    rows, g, _bad = gr.sparse_grad(DRIFT_ROWS, ids, off, G)
    for t in range(DRIFT_STEPS):
        if stochastic:
            table, _s = step_rows("bf16", table, None, rows, g, "sgd", DRIFT_LR, 0.0, DRIFT_SEED, t)
        else:
            table = gr.sgd_step("bf16", table, rows, g, DRIFT_LR)
        out.append(table)
    return out


def ulps_above_one(table_bytes):
    """The total of bf16 ulps (2^-7 each) the elements of a table in [1, 2) lie above 1.0."""
    b = np.ascontiguousarray(table_bytes).view(np.uint16).astype(np.int64)
    assert ((b >= 0x3F80) & (b < 0x4000)).all()
    return int((b - 0x3F80).sum())
