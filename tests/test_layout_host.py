"""The LDS / workspace layouts of the chain kernels (csrc/mpp_layout.hpp) are what they were before each was written once.

tests/layout_walk.hip is compiled for the host with -fsanitize=address,undefined and run as a program: it walks the pointer
walkers over host buffers of exactly the counted size, writes every array end to end, and prints sizes and offsets.  The
yardstick is independent of the header: the closed-form byte counts (lds_bytes, hbm_state_bytes, hbm_lds_bytes,
deep_extra_bytes, deep_base_bytes) and the pointer walks (carve, carve_hbm, deep_carve) of the commit before the layouts
were unified, restated below in Python.
"""
import os
import subprocess

import pytest

from mpp_cnn_rs_object_detection_amd import build as mpp_build

HERE = os.path.dirname(os.path.abspath(__file__))
NCLASS, STASH, CLIP_SLOTS, DEEP_CLIST, HBM_ALIGN = 32, 32, 4, 192, 256
SIZEOF_REC = 18 * 4 + 20 * 8        # struct Rec: 18 ints, 20 doubles
D, I, H, B, U4 = 8, 4, 2, 1, 16     # double, int, unsigned short, unsigned char, uint4

CAPS = [1, 7, 64, 65, 1024, 65535]
CELLS = [(1, 1), (9, 7), (256, 64), (64, 2048)]
SPECS = [0, 1, 8, 16, 64]
ROWS = [0, 65, 1025]
WAVES = [1, 4, 8, 16]
NMAX = [8, 128, 256]


def up(b, a):
    return (b + a - 1) & ~(a - 1)


# ---- the former closed forms ------------------------------------------------------------------------------------------
def old_lds_bytes(cap, ncell, cell_cap, spec, rowbase_n, waves):
    b = waves * CLIP_SLOTS * 32 * D
    b += 11 * cap * D
    b += rowbase_n * D
    b += 3 * NCLASS * D
    b += 2 * NCLASS * D
    b += 2 * spec * STASH * D
    b += cap * I
    b += cap * H
    b += ncell * cell_cap * H
    b += ncell * H
    b += spec * STASH * H
    b += cap
    b = up(b, 16)
    b += spec * SIZEOF_REC
    b += 16 * I
    return b + 64


def old_hbm_state_bytes(cap, ncell, cell_cap):
    a = lambda b: up(b, HBM_ALIGN)
    return 11 * a(cap * D) + a(cap * I) + a(cap * H) + a(ncell * cell_cap * H) + a(ncell * H) + a(cap)


def old_hbm_lds_bytes(spec, rowbase_n, waves):
    b = waves * CLIP_SLOTS * 32 * D
    b += rowbase_n * D
    b += 5 * NCLASS * D
    b += 2 * spec * STASH * D
    b += spec * STASH * H
    b = up(b, 16)
    b += spec * SIZEOF_REC
    b += 16 * I
    return b + 64


def old_deep_extra_bytes(nmax, waves, ext):
    return (nmax * 16 + 4 * nmax * 8 + waves * (2 + (1 if ext else 0)) * 64 * 8 + waves * DEEP_CLIST * 4 + nmax * 32 + nmax * 40 +
            nmax * 2 + waves * 16 * 2 + waves * 128 + 64)


def old_deep_base_bytes(cap, ncell, cell_cap, rowbase_n, waves):
    return up(old_lds_bytes(cap, ncell, cell_cap, 0, rowbase_n, waves), 16)


# ---- the former pointer walks: name -> (offset or None, elements, element size) ---------------------------------------
def old_carve(cap, ncell, cell_cap, spec, rowbase_n, waves):
    out, d = {}, 0
    for name in ["s", "r", "a", "ca", "sa", "hl", "hw", "rad", "lin", "red0", "red1"]:
        out[name] = (d, cap, D); d += cap * D
    out["edges"] = (d, 3 * NCLASS, D); d += 3 * NCLASS * D
    out["trig"] = (d, 2 * NCLASS, D); d += 2 * NCLASS * D
    out["rowbase"] = (d if rowbase_n > 0 else None, rowbase_n, D); d += rowbase_n * D
    out["stash_v0"] = (d, spec * STASH, D); d += spec * STASH * D
    out["stash_v1"] = (d, spec * STASH, D); d += spec * STASH * D
    out["clip"] = (d, waves * CLIP_SLOTS * 32, D); d += waves * CLIP_SLOTS * 32 * D
    out["xy"] = (d, cap, I)
    u = d + cap * I
    out["order"] = (u, cap, H); u += cap * H
    out["cell_items"] = (u, ncell * cell_cap, H); u += ncell * cell_cap * H
    out["cell_cnt"] = (u, ncell, H); u += ncell * H
    out["stash_slot"] = (u, spec * STASH, H); u += spec * STASH * H
    out["gate"] = (u, cap, B)
    off = up(u + cap, 16)
    out["rec"] = (off, spec, SIZEOF_REC)
    out["sh"] = (off + spec * SIZEOF_REC, 16, I)
    return out


def old_carve_hbm_state(cap, ncell, cell_cap):
    a = lambda b: up(b, HBM_ALIGN)
    out, dc = {}, a(cap * D)
    for k, name in enumerate(["s", "r", "a", "ca", "sa", "hl", "hw", "rad", "lin", "red0", "red1"]):
        out[name] = (k * dc, cap, D)
    o = 11 * dc
    out["xy"] = (o, cap, I); o += a(cap * I)
    out["order"] = (o, cap, H); o += a(cap * H)
    out["cell_items"] = (o, ncell * cell_cap, H); o += a(ncell * cell_cap * H)
    out["cell_cnt"] = (o, ncell, H); o += a(ncell * H)
    out["gate"] = (o, cap, B)
    return out


def old_carve_hbm_lds(spec, rowbase_n, waves):
    out, d = {}, 0
    out["edges"] = (d, 3 * NCLASS, D); d += 3 * NCLASS * D
    out["trig"] = (d, 2 * NCLASS, D); d += 2 * NCLASS * D
    out["rowbase"] = (d if rowbase_n > 0 else None, rowbase_n, D); d += rowbase_n * D
    out["stash_v0"] = (d, spec * STASH, D); d += spec * STASH * D
    out["stash_v1"] = (d, spec * STASH, D); d += spec * STASH * D
    out["clip"] = (d, waves * CLIP_SLOTS * 32, D); d += waves * CLIP_SLOTS * 32 * D
    out["stash_slot"] = (d, spec * STASH, H); d += spec * STASH * H
    off = up(d, 16)
    out["rec"] = (off, spec, SIZEOF_REC)
    out["sh"] = (off + spec * SIZEOF_REC, 16, I)
    return out


def old_deep_carve(base, nmax, waves, ext):
    out = {}
    out["pw"] = (base, nmax, U4); base += nmax * 16
    out["tring"] = (base, 4 * nmax, D); base += 4 * nmax * 8
    nr = waves * (2 + (1 if ext else 0)) * 64
    out["racc"] = (base, nr, 8); base += nr * 8
    out["clist"] = (base, waves * DEEP_CLIST, 4); base += waves * DEEP_CLIST * 4
    out["info"] = (base, nmax, U4); base += nmax * 16
    out["nb"] = (base, nmax, U4); base += nmax * 16
    out["st"] = (base, 5 * nmax, D); base += nmax * 40
    out["poff"] = (base, nmax, H); base += nmax * 2
    out["tcnt"] = (base, waves * 16, H); base += waves * 16 * 2
    out["ltab"] = (base, waves * 128, B)
    return out


# ---- the program ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """The program's output, one parsed record per line: (layout, {shape key: value}, {array: (offset, n, elem)})."""
    exe = str(tmp_path_factory.mktemp("layout") / "layout_walk")
    cmd = [mpp_build.HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(HERE, "layout_walk.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[0] == "sizeof Rec=%d uint4=16" % SIZEOF_REC
    recs = []
    for line in lines[1:]:
        parts = line.split()
        shape, arrays = {}, {}
        for p in parts[1:]:
            k, v = p.split("=")
            if ":" in v:
                off, n, elem = (int(x) for x in v.split(":"))
                arrays[k] = (None if off < 0 else off, n, elem)
            else:
                shape[k] = int(v)
        recs.append((parts[0], shape, arrays))
    return recs


def check_arrays(arrays, want, size, align_of):
    """(b) offsets and lengths are the former ones; (c) disjoint, inside the buffer, aligned; (d) rowbase."""
    assert list(arrays) == list(want)                       # the same arrays, in memory order
    spans = []
    for name, (off, n, elem) in arrays.items():
        assert (off, n, elem) == want[name], name
        if off is None:
            continue
        assert off % align_of(name, elem) == 0, name
        assert 0 <= off and off + n * elem <= size, name
        if n:
            spans.append((off, off + n * elem))
    spans.sort()
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0


def lds_align(name, elem):
    return 16 if elem in (SIZEOF_REC, U4) else elem           # Rec and uint4: 16 bytes


def test_every_shape_was_walked(walk):
    seen = {}
    for layout, shape, _ in walk:
        seen.setdefault(layout, set()).add(tuple(sorted(shape.items())))
    n_chain = len(CAPS) * len(CELLS) * len(SPECS) * len(ROWS) * len(WAVES)
    n_base = len(CAPS) * len(CELLS) * len(ROWS) * len(WAVES)
    assert len(seen["chain"]) == n_chain
    assert len(seen["deep_chain"]) == n_base
    assert len(seen["deep"]) == n_base * len(NMAX) * 2
    assert len(seen["hbm_state"]) == len(CAPS) * len(CELLS)
    assert len(seen["hbm_lds"]) == len(SPECS) * len(ROWS) * len(WAVES)
    for layout, shape, _ in walk:                           # ... and they are the shapes of the lists above
        assert shape.get("cap", CAPS[0]) in CAPS and (shape.get("ncell", 1), shape.get("cell_cap", 1)) in CELLS
        assert shape.get("spec", 0) in SPECS and shape.get("rowbase_n", 0) in ROWS and shape.get("waves", 1) in WAVES
        assert shape.get("nmax", NMAX[0]) in NMAX and shape.get("ext", 0) in (0, 1)


def test_chain_layout(walk):
    n = 0
    for layout, s, arrays in walk:
        if layout not in ("chain", "deep_chain"):
            continue
        key = (s["cap"], s["ncell"], s["cell_cap"], s["spec"], s["rowbase_n"], s["waves"])
        size = old_lds_bytes(*key) if layout == "chain" else old_deep_base_bytes(*key[:3], *key[4:])
        assert s["bytes"] == size, key
        check_arrays(arrays, old_carve(*key), old_lds_bytes(*key), lds_align)
        assert (arrays["rowbase"][0] is None) == (s["rowbase_n"] == 0)
        n += 1
    assert n > 0


def test_hbm_layout(walk):
    n = 0
    for layout, s, arrays in walk:
        if layout == "hbm_state":
            key = (s["cap"], s["ncell"], s["cell_cap"])
            assert s["bytes"] == old_hbm_state_bytes(*key), key
            check_arrays(arrays, old_carve_hbm_state(*key), s["bytes"], lambda name, elem: HBM_ALIGN)
            n += 1
        elif layout == "hbm_lds":
            key = (s["spec"], s["rowbase_n"], s["waves"])
            assert s["bytes"] == old_hbm_lds_bytes(*key), key
            check_arrays(arrays, old_carve_hbm_lds(*key), s["bytes"], lds_align)
            assert (arrays["rowbase"][0] is None) == (s["rowbase_n"] == 0)
            n += 1
    assert n == len(CAPS) * len(CELLS) + len(SPECS) * len(ROWS) * len(WAVES)


def test_deep_layout(walk):
    n = 0
    for layout, s, arrays in walk:
        if layout != "deep":
            continue
        base = old_deep_base_bytes(s["cap"], s["ncell"], s["cell_cap"], s["rowbase_n"], s["waves"])
        assert s["base"] == base and base % 16 == 0
        assert s["bytes"] == base + old_deep_extra_bytes(s["nmax"], s["waves"], s["ext"])
        check_arrays(arrays, old_deep_carve(base, s["nmax"], s["waves"], s["ext"]), s["bytes"], lds_align)
        assert min(off for off, _, _ in arrays.values()) >= old_lds_bytes(s["cap"], s["ncell"], s["cell_cap"], 0, s["rowbase_n"], s["waves"])
        n += 1
    assert n == len(CAPS) * len(CELLS) * len(ROWS) * len(WAVES) * len(NMAX) * 2

