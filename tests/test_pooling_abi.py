"""CPU: the pooled-lookup surface of the C ABI (emb_pool_spec, emb_lookup_pooled, emb_plan_create_pooled) -- layout against
the header as gcc lays it out, constants, exports -- and the bag_pool_* kernels in the gfx950 code object: present for every
path, none spilling, and every pooled launch record naming exactly one of them."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pimemb.h")


def test_pool_spec_layout_matches_the_header(pel, tmp_path):
    L = pel.lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pimemb.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(emb_pool_spec));']
    for fname, _ in L.EmbPoolSpec._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(emb_pool_spec, %s));' % (fname, fname))
    lines.append("return 0;}")
    src = tmp_path / "pool_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "pool_layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(L.EmbPoolSpec) == 24
    for fname, _ in L.EmbPoolSpec._fields_:
        assert int(got[fname]) == getattr(L.EmbPoolSpec, fname).offset, fname


def test_pool_constants_match_the_header(pel):
    text = open(HEADER).read()
    L = pel.lib
    for name in ("EMB_POOL_SUM", "EMB_POOL_MEAN", "EMB_POOL_MAX", "EMB_POOL_PADDING"):
        assert re.search(r"#define %s %du\b" % (name, getattr(L, name)), text), name
    assert len({L.EMB_POOL_SUM, L.EMB_POOL_MEAN, L.EMB_POOL_MAX}) == 3


def test_library_exports_the_pooled_entry_points(pel):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pel.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"emb_lookup_pooled", "emb_plan_create_pooled"} <= exported
    assert {"emb_lookup_pooled", "emb_plan_create_pooled"} <= set(pel.lib.SIGNATURES)
    L = pel.lib.load()
    assert L.emb_lookup_pooled is not None and L.emb_plan_create_pooled is not None


def test_pool_kernels_are_in_the_code_object_and_do_not_spill(pel):
    from pim_embedding_lookup_amd import codeobj
    res = codeobj.kernel_resources(pel.LIB_PATH)
    pooled = {k: r for k, r in res.items() if "bag_pool_" in k}
    for family in ("bag_pool_group_kernel", "bag_pool_wavebatch_kernel", "bag_pool_anydim_kernel"):
        assert any(family in k for k in pooled), family
    # index width x {fp32, fp16} x 7 row widths x 2 paths + index width x {fp32, fp16} x {element, piece}
    assert len(pooled) == 2 * 2 * 7 * 2 + 2 * 2 * 2
    spilling = {k: r for k, r in pooled.items() if r["vgpr_spill"] or r["sgpr_spill"] or r["scratch"]}
    assert not spilling, spilling


def test_every_pooled_launch_record_names_one_kernel(pel):
    """codeobj.symbol_fragments for the records emb_plan_describe writes for pooled launches (no GPU needed: the records are
    built by hand for every path, index width, dtype and row width)."""
    from pim_embedding_lookup_amd import codeobj
    hashes = codeobj.kernel_hashes(pel.LIB_PATH)
    for itype in (0, 1):
        for dtype in (0, 1):
            for kind in (0, 1):
                for lpr in (1, 2, 4, 8, 16, 32, 64):
                    rec = dict(kind=kind, dtype=dtype, itype=itype, lanes_per_row=lpr, anydim_vec=0, ranged=0, pool=1)
                    frags = codeobj.symbol_fragments(rec)
                    hits = [k for k in hashes if all(f in k for f in frags)]
                    assert len(hits) == 1, (rec, hits)
                    assert "bag_pool_" in hits[0]
            for vec in (0, 1):
                rec = dict(kind=3, dtype=dtype, itype=itype, lanes_per_row=0, anydim_vec=vec, ranged=0, pool=2)
                hits = [k for k in hashes if all(f in k for f in codeobj.symbol_fragments(rec))]
                assert len(hits) == 1 and "bag_pool_anydim" in hits[0], (rec, hits)
