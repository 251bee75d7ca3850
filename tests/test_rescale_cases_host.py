"""The rescale edge cases without a GPU (``rescale_cases.py``): the references agree with each other, every case reaches the
branch of the kernels it is there for (counted by ``rescale_cases.plan``, the Python restatement of the launcher's checks and
of the addresses ``k_rescale_rows`` forms), the reference alone settles the 8-bit level of all but 0.1 % of the values, and
the refusals of the tables' builder name what was asked.  ``pytest -s`` prints the rows of profiles/rescale_edge_tests.md."""
import numpy as np
import pytest

import rescale_cases as RC
import rescale_ref as R
from mpp_cnn_rs_object_detection_amd import dataset_translation as dt
from mpp_cnn_rs_object_detection_amd import detect

#: the first byte of the source: on a 16-byte boundary (torch's own allocations), and 5 bytes past one
BASES = (0, 5)

#: count -> the cases that are there for it (``plan`` with base 0 unless the count names another)
REACHES = {
    "partial_groups": ["1x1@1", "5x7@0.5", "17x126@0.5", "31x130@0.5", "64x1400@0.0936", "generic 37x150->21x71"],
    "lanes_past_ow": ["1x1@1", "300x7@0.2119", "17x126@0.5", "31x130@0.5"],
    "chunks_high": [c.name for c in RC.ALL_CASES if c.name != "64x1400@0.093"],
    "row_blocks_with_tail": ["1x1@1", "5x7@0.5", "17x126@0.5", "33x128@0.5", "31x130@0.5", "15x70@0.5", "22x66@0.5"],
    "threads_live_1": ["1x1@1", "5x7@0.5", "17x126@0.5", "33x128@0.5", "1x200->1x100"],
    "threads_live_2": ["2x2@0.5", "22x66@0.5", "50x50@0.99"],
    "threads_live_3": ["3x40@0.34", "7x300@0.2119", "31x130@0.5", "15x70@0.5"],
    "odd_ow3": ["9x342@0.5", "1x1@1", "17x126@0.5", "31x130@0.5", "64x1400@0.0936", "generic 37x150->21x71"],
}
#: ... and the cases that must not reach it: the full group, the full row blocks
AVOIDS = {
    "partial_groups": ["33x128@0.5", "7x300@0.2119"],
    "lanes_past_ow": ["33x128@0.5", "7x300@0.2119"],
    "odd_ow3": ["33x128@0.5", "40x1300@0.095"],
    "row_blocks_with_tail": ["16x5@1", "64x1400@0.0936", "400x24->50x24"],
}


def admitted(case):
    return RC.plan(case.H, case.W, case.tables(), addresses=False).refusal is None


RUN_CASES = [c for c in RC.ALL_CASES if admitted(c)]


def test_the_output_shapes_are_the_ones_the_cases_are_named_for():
    shapes = {c.name: c.out for c in RC.ALL_CASES}
    for name, out in (("1x1@1", (1, 1)), ("2x2@0.5", (1, 1)), ("5x7@0.5", (2, 4)), ("3x40@0.34", (1, 14)), ("16x5@1", (16, 5)),
                      ("50x50@0.99", (50, 50)), ("7x300@0.2119", (1, 64)), ("300x7@0.2119", (64, 1)), ("17x126@0.5", (8, 63)),
                      ("33x128@0.5", (16, 64)), ("31x130@0.5", (16, 65)), ("64x1400@0.0936", (6, 131)),
                      ("64x1400@0.093", (6, 130)), ("9x342@0.5", (4, 171)), ("40x1300@0.095", (4, 124))):
        assert shapes[name] == out, name
    taps = {c.name: (c.tables()[0].shape[1], c.tables()[2].shape[1]) for c in RC.ALL_CASES}
    assert taps["7x300@0.2119"] == (26, 16) and taps["300x7@0.2119"] == (16, 26) and taps["16x5@1"] == (2, 2)
    assert taps["24x400->24x50"] == (2, 30) and taps["400x24->50x24"] == (30, 2) and taps["generic 37x150->21x71"] == (3, 5)
    assert [c.name for c in RC.ALL_CASES if c.flat] == ["40x48@0.5"]                     # the flat blocks: one case only
    assert sorted(c.name for c in RC.ALL_CASES if c.pass_through()) == ["16x5@1", "1x1@1", "50x50@0.99"]
    for c in RC.ALL_CASES:
        ri, _, ci, _ = c.tables()
        assert 0 <= ri.min() and ri.max() < c.H and 0 <= ci.min() and ci.max() < c.W


@pytest.mark.parametrize("case", [c for c in RC.ALL_CASES if c.gaussian], ids=repr)
def test_apply_tables_of_the_projects_tables_is_the_restatement(case):
    """1e-12, the bound of ``test_tables_reproduce_the_scipy_restatement``: at most 42 x 42 terms of size <= 1 at 1.1e-16 give
    2e-13.  The refused case has no device result, but its tables are as good as the others'."""
    err = float(np.abs(R.apply_tables(case.image(), *case.tables()) - case.reference()).max())
    print(f"{case.name}: max |apply_tables - restatement| = {err:.3g}")
    assert err <= 1e-12
    for w in (case.tables()[1], case.tables()[3]):
        assert np.abs(w.sum(axis=1) - 1).max() <= 1e-15 and w.min() >= 0


def test_resize_ref_with_the_shape_of_a_scale_is_rescale_ref():
    for c in (RC.BY_NAME["31x130@0.5"], RC.BY_NAME["3x40@0.34"]):
        assert np.array_equal(R.resize_ref(c.image(), *c.out), R.rescale_ref(c.image(), c.scale))


def test_generic_tables_float64_against_longdouble_and_the_clip_acts():
    """float64 ``apply_tables`` within the device's own tolerance of the longdouble evaluation (NumPy's pairwise sums of
    Tr Tc terms stay under the term-count bound as the kernels' chains do); by the longdouble reference alone, at least 10 %
    of the values lie below 0 and at least 10 % above 1."""
    c = RC.GENERIC
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no wider than float64 here"
    ri, rw, ci, cw = c.tables()
    assert rw.min() < -0.4 and rw.max() > 0.9 and np.abs(rw).max() <= 1 and np.abs(cw).max() <= 1
    assert (np.diff(ci[:, 0]) < 0).any() and (np.diff(ri[:, 0]) < 0).any()                 # not monotone
    exact = R.apply_tables(c.image(), *c.tables(), dtype=np.longdouble)
    err = float(np.abs(R.apply_tables(c.image(), *c.tables()) - exact).max())
    below, above = float((exact < 0).mean()), float((exact > 1).mean())
    print(f"{c.name}: tolerance {c.tolerance():.3g}, max |float64 - longdouble| = {err:.3g}; {below:.1%} below 0, {above:.1%} above 1")
    assert err <= c.tolerance()
    assert below >= 0.10 and above >= 0.10
    assert RC.plan(c.H, c.W, c.tables()).span == c.W                                      # a group spans the whole width


@pytest.mark.parametrize("case", RUN_CASES, ids=repr)
def test_a_case_reaches_its_branches(case):
    """the counts of ``plan`` (which also asserts, for every row and group, that the bytes the taps name lie inside the image
    and inside the staged span), at both placements of the source"""
    plans = {b: RC.plan(case.H, case.W, case.tables(), base=b) for b in BASES}
    n = plans[0].counts
    for key, names in REACHES.items():
        if case.name in names:
            assert n[key] > 0, (key, n)
    for key, names in AVOIDS.items():
        if case.name in names:
            assert n[key] == 0, (key, n)
    # a source off the 16-byte grid: the first chunk of the first row begins below the image
    assert n["chunks_low"] == 0 and plans[5].counts["chunks_low"] > 0 and plans[5].counts["chunks_high"] > 0
    assert plans[0].bands == plans[5].bands == [(0, case.out[0], plans[0].bands[0][2], plans[0].bands[0][3])]
    assert (n["cols_blocks"], n["cols_threads_in_last_block"]) == ((2, 1) if case.name == "9x342@0.5" else (1, (3 * case.out[1] + 1) // 2))
    folded = 0
    if case.gaussian:
        folded = RC.taps_folded_twice(case.H, case.out[0]) + RC.taps_folded_twice(case.W, case.out[1])
    if case.name in ("3x40@0.34", "2x2@0.5", "1x200->1x100"):
        assert folded > 0
    ref = case.reference()
    clipped = int(((ref < 0) | (ref > 1)).sum())
    assert (clipped > 0) == (not case.gaussian)
    print(f"| `{case.name}` | {case.out[0]} x {case.out[1]} | {plans[0].shape[2]} / {plans[0].shape[3]} | {plans[0].lds} | "
          f"{n['groups']} ({n['partial_groups']}) | {n['lanes_past_ow']} | {n['chunks_inside']} / {n['chunks_low']} / {n['chunks_high']} | "
          f"{plans[5].counts['chunks_inside']} / {plans[5].counts['chunks_low']} / {plans[5].counts['chunks_high']} | "
          f"{n['row_blocks']} ({n['row_blocks_with_tail']}) | {n['threads_live_1'] // 64} / {n['threads_live_2'] // 64} / "
          f"{n['threads_live_3'] // 64} / {n['threads_live_0'] // 64} | {n['odd_ow3']} | {len(n['residues'])} / "
          f"{len(plans[5].counts['residues'])} | {n['cols_blocks']} ({n['cols_threads_in_last_block']}) | {folded} | {clipped} |")


def test_16x5_folds_the_tap_at_n_in_back_with_weight_zero():
    ri, rw, ci, cw = RC.BY_NAME["16x5@1"].tables()
    assert ri[-1].tolist() == [15, 14] and rw[-1].tolist() == [1.0, 0.0] and ci[-1].tolist() == [4, 3] and cw[-1].tolist() == [1.0, 0.0]


def test_row_counts_per_band():
    """1, 15, 16 and 17 source rows in one band; rows mod 16 = 1, 1, 15 at the column-group cases"""
    rows = {c.name: RC.plan(c.H, c.W, c.tables(), addresses=False).bands for c in RUN_CASES}
    assert rows["1x1@1"] == [(0, 1, 0, 1)] and rows["15x70@0.5"][0][2:] == (0, 15) and rows["16x5@1"][0][2:] == (0, 16)
    assert rows["17x126@0.5"][0][2:] == (0, 17) and rows["33x128@0.5"][0][2:] == (0, 33) and rows["31x130@0.5"][0][2:] == (0, 31)


def test_the_lds_limit_has_cases_on_both_sides():
    """the bytes by the launcher's formula: 8 + 4 bytes per tap and lane, 16 for the minimum and maximum, 16 rows of the span
    rounded to whole chunks with room for 15 bytes of misalignment"""
    seen = {}
    for name in ("64x1400@0.0936", "64x1400@0.093", "40x1300@0.095"):
        c = RC.BY_NAME[name]
        q = RC.plan(c.H, c.W, c.tables(), addresses=False)
        Tc = c.tables()[2].shape[1]
        stride = -(-(3 * q.span + 15) // 16) * 16
        lds = 768 * Tc + 16 + 16 * stride
        assert lds == q.lds and stride == q.row_stride
        seen[name] = (lds, q.refusal)
        print(f"{name}: Tc {Tc}, span {q.span}, row stride {stride}, {lds} bytes of LDS: {'refused' if q.refusal else 'admitted'}")
        assert (q.refusal == "LDS") == (lds > RC.RS_LDS_MAX)
    verdicts = [r for _, r in seen.values()]
    assert None in verdicts and "LDS" in verdicts
    # the nearest cases on each side are within 2 KiB of the limit
    assert max(b for b, r in seen.values() if r is None) > RC.RS_LDS_MAX - 2048
    assert min(b for b, r in seen.values() if r) < RC.RS_LDS_MAX + 2048


@pytest.mark.parametrize("case", RUN_CASES, ids=repr)
def test_the_reference_settles_the_8_bit_level(case):
    """the share of values whose 255 clip(ref) lies within 255 tol of an integer: at most 0.1 % for pure noise.  Exempt: the
    flat-block case (there the levels may differ by one), and the three pass-through cases, where every value is a byte / 255
    whatever the seed -- and where, every weight being 0 or 1, the device's value is that same quotient, so the GPU test
    compares all of their levels instead of none."""
    share = float(RC.excluded(case.reference(), case.tolerance()).mean())
    print(f"{case.name}: {share:.4%} of {case.reference().size} values within {255 * case.tolerance():.3g} of a level")
    if case.pass_through():
        assert share == 1.0
    elif not case.flat:
        assert share <= 0.001
    else:
        assert share > 0.05                                  # the flat blocks do what they are there for


def test_alignment_sweep_reaches_every_residue_and_pattern():
    c = RC.ALIGN
    W3 = 3 * c.W
    patterns = {}
    for pitch in RC.ALIGN_PITCHES:
        assert pitch >= W3
        per_base = []
        for base in range(16):
            n = RC.plan(c.H, c.W, c.tables(), pitch=pitch, base=base).counts
            per_base.append(len(n["residues"]))
            assert (n["chunks_low"] > 0) == (base > 0) and n["chunks_high"] > 0
        patterns[pitch] = max(per_base)
    print("distinct residues of (address & 15) per pitch:", patterns)
    assert [W3, W3 + 1, W3 + 8, W3 + 16] == list(RC.ALIGN_PITCHES[:4])
    assert patterns[W3 + 1] == 16                            # a residue that changes with every row
    assert sorted(patterns.values())[:2] == [2, 4]           # two groups: fixed (pitch = 0 mod 16), alternating (8 mod 16)


def test_bands_at_the_group_edges():
    """a limit that forces at least 3 bands, and one that leaves a single source row of slack over the one-band need"""
    for name in ("17x126@0.5", "31x130@0.5"):
        c = RC.BY_NAME[name]
        one = RC.plan(c.H, c.W, c.tables(), addresses=False)
        assert len(one.bands) == 1
        tight = RC.plan(c.H, c.W, c.tables(), ws_limit=RC.band_limit(c, RC.BAND_ROWS))
        assert len(tight.bands) >= 3 and max(tight.counts["band_rows"]) <= RC.BAND_ROWS
        assert [b[:2] for b in tight.bands][0][0] == 0 and tight.bands[-1][1] == c.out[0]
        slack = RC.plan(c.H, c.W, c.tables(), ws_limit=one.need + one.row_bytes, addresses=False)
        short = RC.plan(c.H, c.W, c.tables(), ws_limit=one.need - 1, addresses=False)
        assert len(slack.bands) == 1 and len(short.bands) == 2
        print(f"{name}: one band needs {one.need} bytes ({one.tab_bytes} of tables, {one.row_bytes} per row); "
              f"{RC.BAND_ROWS} rows: {len(tight.bands)} bands of {tight.counts['band_rows']} rows; one byte short: "
              f"{[b[3] - b[2] for b in short.bands]} rows")
    q = RC.plan(c.H, c.W, c.tables(), ws_limit=one.tab_bytes + one.row_bytes - 1)
    assert q.refusal == "workspace"


def test_refusals_of_the_restated_launcher():
    c = RC.ALIGN
    ri, rw, ci, cw = c.tables()
    assert RC.plan(c.H, c.W, (ri + np.int32(c.H) * (ri == ri.max()), rw, ci, cw)).refusal == "outside"
    wide = (np.zeros((1, RC.RS_MAX_TAPS + 1), np.int32), np.zeros((1, RC.RS_MAX_TAPS + 1)), ci, cw)
    assert RC.plan(c.H, c.W, wide).refusal == "taps"


# ---- a picture too small for its scale ---------------------------------------------------------------------------------------
def test_a_picture_that_rounds_to_no_rows_is_refused_by_name():
    with pytest.raises(ValueError, match=r"1 x 200 .*0\.5.*0 x 100"):
        dt.rescale_image_tables(1, 200, 0.5)
    with pytest.raises(ValueError, match=r"3 x 2 .*0\.1"):
        dt.rescale_image_tables(3, 2, 0.1)
    with pytest.raises(ValueError, match="not a reduction"):                # the per-axis builder keeps its own words
        dt.rescale_tables(1, 0)

    class WithNets:
        nets, device = object(), 0

    with pytest.raises(ValueError, match=r"1 x 200 .*0\.5"):              # what detect shows for --gsd 0.25 on such a file
        detect.detect_image(WithNets(), np.zeros((1, 200, 3), np.uint8), gsd=0.25, model_gsd=0.5)
    (oh, ow), _ = dt.rescale_image_tables(2, 200, 0.5)
    assert (oh, ow) == (1, 100)
