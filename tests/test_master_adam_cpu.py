"""CPU: the fused master-weight Adam steps (include/pimemb_grad.h, THE MASTER-WEIGHT ADAM STEPS).  The new entry point is declared, exported,
bound and linked as the header says and refuses what it says; the new code object holds the shipped kernels and nothing else, with no
scratch, no spills and no LDS; tests/master_adam_ref.py equals the composition it stands for.  No GPU work is called."""
import ctypes as C
import os
import subprocess
import sys
import threading
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as ar  # noqa: E402
import grad_ref as gr  # noqa: E402
import master_adam_ref as mar  # noqa: E402
import rows_cases as rc  # noqa: E402
import train_ref as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAME = "emb_grad_master_adam_step"


def test_declared_exported_bound_and_linked(pel):
    build = import_module("pim-embedding-lookup_amd.build")
    header = open(os.path.join(ROOT, "include", "pimemb_grad.h")).read()
    assert "THE MASTER-WEIGHT ADAM STEPS" in header and NAME + "(" in header
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.GRAD_LIB_PATH], text=True)
    assert NAME in {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert getattr(pel.lib.load_grad(), NAME).argtypes == pel.lib.GRAD_SIGNATURES[NAME][1] and len(pel.lib.GRAD_SIGNATURES[NAME][1]) == 9
    dyn = subprocess.check_output(["readelf", "-d", build.GRAD_LIB_PATH], text=True)
    assert "libpimemb_grad_master_adam.so" in dyn and "$ORIGIN" in dyn
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.GRAD_MASTER_ADAM_LIB_PATH], text=True)
    assert "pimemb_grad_master_adam_launch" in {line.split()[-1] for line in syms.splitlines()}


def refusals(pel):
    G = pel.lib.load_grad()
    INV = pel.lib.EMB_ERR_INVALID
    d, ptrs, err = pel.lib.EmbGradDesc(), (C.c_void_p * 1)(), G.emb_grad_last_error
    good = dict(kind=1, eps=1e-8, lr=0.1, beta1=0.9, beta2=0.999, step=1, step_size_dev=None, reserved=0)
    spec = lambda **kw: C.byref(pel.lib.EmbAdamSpec(**{**good, **kw}))  # noqa: E731
    step = getattr(G, NAME)
    assert step(None, C.byref(d), ptrs, ptrs, ptrs, 1, 0, spec(), None) == INV and b"context is NULL" in err()
    # the Adam step's texts, before the context is looked at
    for kw, text in ((dict(kind=0), b"unknown Adam kind"), (dict(kind=3), b"unknown Adam kind"), (dict(reserved=1), b"reserved field must be 0"),
                     (dict(beta1=1.0), b"must lie in [0, 1)"), (dict(eps=-1.0), b"eps must not be negative"), (dict(lr=float("inf")), b"lr must be finite"),
                     (dict(step=0), b"step counts from 1"), (dict(step_size_dev=6), b"not 4-byte aligned")):
        assert step(None, C.byref(d), ptrs, ptrs, ptrs, 1, 0, spec(**kw), None) == INV and text in err(), kw
    assert step(None, C.byref(d), ptrs, ptrs, ptrs, 1, 0, None, None) == INV and b"spec is NULL" in err()
    fake = C.c_void_p(16)
    for args in ((None, ptrs, ptrs), (ptrs, None, ptrs), (ptrs, ptrs, None)):
        assert step(fake, C.byref(d), *args, 1, 0, spec(), None) == INV and b"is NULL" in err()
    assert step(fake, C.byref(d), ptrs, ptrs, ptrs, 1, 7, spec(), None) == INV and b"index type" in err()


def test_refusals_of_bad_specs_and_of_a_null_context(pel):
    """On a thread of its own, as in tests/test_adam_cpu.py: emb_grad_last_error is thread-local and never cleared."""
    failed = ["the thread did not finish"]
    t = threading.Thread(target=lambda: refusals(pel) or failed.clear(), daemon=True)
    t.start()
    t.join()
    assert not failed, failed


def test_the_kernels_have_a_code_object_of_their_own_and_use_no_scratch():
    codeobj = import_module("pim-embedding-lookup_amd.codeobj")
    build = import_module("pim-embedding-lookup_amd.build")
    res = codeobj.kernel_resources(build.GRAD_MASTER_ADAM_LIB_PATH)
    inst = lambda name, *args: "%d%sIL" % (len(name), name) + "EL".join(args) + "EEE"  # noqa: E731
    want = [inst("grad_master_adam_rows_group", "i%d" % k, "b%d" % s) for k in (1, 2) for s in (0, 1)]
    want += [inst("grad_master_adam_rows_elem", "b%d" % s) for s in (0, 1)]
    assert len(res) == 6 and all(sum(w in k for k in res) == 1 for w in want), sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, (k, v)


@pytest.mark.parametrize("rowwise", [False, True])
@pytest.mark.parametrize("kind", mar.KINDS)
def test_the_reference_equals_its_composition(kind, rowwise):
    """grad_ref's sparse gradient -> adam_ref's values on the master rows -> host_encode of the new master: written out here, once per dtype."""
    dim, lr, betas, eps = 32, 0.05, (0.5, 0.9), 1e-6
    st = tr.initial_state(kind, dim)
    b, G = tr.train_batches(kind, dim, 1)[0]
    ids, off, mode, w, pad = b.args("weighted+pad", "i64")
    table, master = st.table, st.master
    m, v = mar.initial_moments(tr.N_ROWS, dim, rowwise)
    for t in (1, 2):
        rows, g, n_bad = gr.sparse_grad(tr.N_ROWS, ids, off, G, mode, w, pad)
        want_p, want_m, want_v = master.copy(), m.copy(), v.copy()
        om1, om2, ss = ar.constants(lr, betas, t)
        for k, r in enumerate(rows):
            if rowwise:
                want_p[r], want_m[r], want_v[r] = ar.rowwise_values(master[r], g[k], m[r], v[r], om1, om2, ss, eps)
            else:
                want_p[r], want_m[r], want_v[r], _x = ar.adam_values(master[r], g[k], m[r], v[r], om1, om2, ss, eps)
        want_table = table.copy()
        want_table[rows] = rc.host_encode(kind, want_p)[rows]
        table, master, m, v, got_rows, got_bad, unenc = mar.master_adam_step(kind, table, master, m, v, ids, off, G, mode, w, pad, lr, betas, eps, t, rowwise)
        assert np.array_equal(got_rows, rows) and got_bad == n_bad == 3 and unenc == 0 and len(rows) > 60
        for got, want in ((master, want_p), (m, want_m), (v, want_v)):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(table, want_table)
    assert not np.array_equal(master, st.master) and m.any() and v.any()
