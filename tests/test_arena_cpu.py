"""tests/arena.py over CPU tensors, driven by small numpy "kernels": each way a kernel can leave its declared reads and
writes must be caught, with a message that names the view and the offset, and a clean kernel must pass.  This is the only
place a wrong kernel is simulated."""
import numpy as np
import pytest

import arena as A

N = 100


def make(align=16, misalign=0):
    """src [N] float32 -> dst [N] float32, the kernel is dst = 2 * src."""
    ar = A.Arena(4 * A.MIN_BAND, device="cpu")
    src_host = np.linspace(-3.0, 5.0, N).astype(np.float32)
    src = ar.input(src_host, align=align, misalign=misalign, name="src")
    dst = ar.output((N,), np.float32, align=align, misalign=misalign, name="dst")
    return ar, src_host, src, dst


def words(ar):
    """The whole arena as numpy float32 words sharing its memory: what a kernel with a wrong index reaches."""
    return ar.words.numpy().view(np.float32)


def word_of(ar, name):
    return ar.view(name).offset // 4


def clean(ar):
    w = words(ar)
    s, d = word_of(ar, "src"), word_of(ar, "dst")
    w[d:d + N] = 2.0 * w[s:s + N]


def test_canary_is_a_usable_poison():
    c = A.canary_words(0, 1 << 16)
    f = c.view(np.float32)
    assert np.isfinite(f).all() and not (f == np.float32(A.oracle_binding.AIR_DIST)).any() and not (f == -7.0).any()
    assert len(np.unique(c)) == len(c)  # a canary copied from elsewhere does not match its new position
    ar = A.Arena(4 * A.MIN_BAND, device="cpu")
    assert np.array_equal(ar.words.numpy().view(np.uint32), A.canary_words(0, ar.nbytes // 4))


@pytest.mark.parametrize("align,misalign", [(16, 0), (16, 4), (8, 0), (4, 0), (4, 4)])
def test_views_sit_at_exactly_the_requested_alignment(align, misalign):
    ar, src_host, src, dst = make(align, misalign)
    for t in (src, dst):
        assert (t.data_ptr() - misalign) % align == 0 and (t.data_ptr() - misalign) % (2 * align) == align
        assert t.is_contiguous()
    assert np.array_equal(src.numpy(), src_host)
    s, d = ar.view("src"), ar.view("dst")
    assert s.offset >= ar.band and d.offset - s.end >= ar.band and ar.nbytes - d.end >= ar.band  # bands on both sides
    assert np.array_equal(dst.numpy().view(np.uint32), A.canary_words(d.offset // 4, N))  # outputs keep the canary


def test_clean_kernel_passes():
    ar, src_host, _, _ = make()
    ar.twin(lambda: clean(ar), {"dst": 2.0 * src_host}, kinds=A.POISON_KINDS)


def test_write_one_element_past_an_output_is_caught():
    ar, src_host, _, _ = make()

    def run():
        clean(ar)
        words(ar)[word_of(ar, "dst") + N] = 1.0
    with pytest.raises(A.ArenaError, match=r"above view 'dst': byte 400 relative to its start, 1 past its 400 bytes"):
        ar.twin(run, {"dst": 2.0 * src_host})


def test_write_one_element_before_an_output_is_caught():
    ar, src_host, _, _ = make()

    def run():
        clean(ar)
        words(ar)[word_of(ar, "dst") - 1] = 1.0
    with pytest.raises(A.ArenaError, match=r"below view 'dst': byte -4 relative to its start"):
        ar.twin(run, {"dst": 2.0 * src_host})


def test_skipped_last_element_is_caught():
    ar, src_host, _, _ = make()

    def run():
        w = words(ar)
        s, d = word_of(ar, "src"), word_of(ar, "dst")
        w[d:d + N - 1] = 2.0 * w[s:s + N - 1]
    with pytest.raises(A.ArenaError, match=r"view 'dst': 4 byte\(s\) differ.*4 still hold.*never written.*offsets \[396, 397, 398, 399\]"):
        ar.twin(run, {"dst": 2.0 * src_host})


def test_write_into_an_input_is_caught():
    ar, src_host, _, _ = make()

    def run():
        clean(ar)
        words(ar)[word_of(ar, "src") + 7] = 0.0
    with pytest.raises(A.ArenaError, match=r"in another view: input 'src' at byte 28 of 400"):
        ar.twin(run, {"dst": 2.0 * src_host})


def test_result_that_depends_on_a_guard_word_is_caught():
    """A read one element past the input: right by accident with one poison, wrong with the other."""
    ar, src_host, _, _ = make()

    def run():
        w = words(ar)
        s, d = word_of(ar, "src"), word_of(ar, "dst")
        w[d:d + N] = 2.0 * w[s:s + N]
        if w[s + N] == np.float32(-1.0):  # decides on the word behind the input
            w[d + N - 1] = 0.0
    with pytest.raises(A.ArenaError, match=r"with poison 'hit' around the views:\nview 'dst'.*offsets \[39[6-9]"):
        ar.twin(run, {"dst": 2.0 * src_host}, kinds=("canary", "hit"))
    ar.twin(run, {"dst": 2.0 * src_host}, kinds=("canary", "air"))  # ... and only the poison that matters shows it


def test_untouched_words_must_keep_the_canary_and_inout_its_upload():
    ar = A.Arena(4 * A.MIN_BAND, device="cpu")
    state = np.arange(40, dtype=np.float32).reshape(10, 4)
    ar.inout(state, name="verts")
    ar.output((10,), np.float32, align=4, name="rows")
    want_v = state.copy()
    want_v[:, 3] = -2.0
    written_v = np.zeros((10, 4), bool)
    written_v[:, 3] = True
    written_r = np.arange(10) >= 3  # rows [3, 10) are rendered

    def run(first_row=3, clobber=False):
        w = words(ar)
        v, r = word_of(ar, "verts"), word_of(ar, "rows")
        w[v + 3:v + 40:4] = -2.0
        w[r + first_row:r + 10] = 9.0
        if clobber:
            w[v + 4] = 77.0
    exp = {"verts": A.Untouched(want_v, written_v), "rows": A.Untouched(np.full(10, 9.0, np.float32), written_r)}
    ar.twin(run, exp)
    with pytest.raises(A.ArenaError, match=r"view 'rows': 4 byte\(s\).*4 lie where the contract leaves the view untouched.*offsets \[8, 9"):
        ar.twin(lambda: run(first_row=2), exp)
    with pytest.raises(A.ArenaError, match=r"view 'verts'.*offsets \[1[6-9].*elements \[\(1, 0\)"):
        ar.twin(lambda: run(clobber=True), exp)


def test_undefined_elements_may_hold_anything_but_stay_inside_the_view():
    """A list with its count: the entries beyond the count are undefined, written or not."""
    ar = A.Arena(4 * A.MIN_BAND, device="cpu")
    ar.output((8,), np.float32, align=4, name="list")
    want = np.array([1, 2, 3, 0, 0, 0, 0, 0], np.float32)
    exp = {"list": A.Untouched(want, undefined=np.arange(8) >= 3)}

    def run(last=5, first_value=1.0):
        w = words(ar)
        w[word_of(ar, "list"):word_of(ar, "list") + last] = [first_value, 2, 3, 9, 9, 9, 9, 9, 9][:last]
    ar.twin(run, exp)
    ar.twin(lambda: run(last=3), exp)
    with pytest.raises(A.ArenaError, match=r"above view 'list'"):
        ar.twin(lambda: run(last=9), exp)
    with pytest.raises(A.ArenaError, match=r"view 'list'.*offsets \[[0-3]"):
        ar.twin(lambda: run(first_value=7.0), exp)


def test_expected_value_equal_to_the_canary_is_refused():
    ar, src_host, _, dst = make()
    want = (2.0 * src_host).astype(np.float32)
    want.view(np.uint32)[5] = A.canary_words(word_of(ar, "dst") + 5, 1)[0]
    with pytest.raises(AssertionError, match="equals the canary at element"):
        ar.twin(lambda: clean(ar), {"dst": want})


def test_a_copy_taken_earlier_is_held_like_the_arena_itself():
    """check(raw=...): what tests/stream_gate.py holds its on-stream snapshot with; poison_of / bytes_of: a view's poison and bytes."""
    ar, src_host, src, dst = make()
    early = ar.raw.clone()                      # before the kernel: dst still holds its canary
    clean(ar)
    late = ar.raw.clone()
    ar.check({"dst": 2.0 * src_host})
    ar.check({"dst": 2.0 * src_host}, raw=late)
    with pytest.raises(A.ArenaError, match="never written"):
        ar.check({"dst": 2.0 * src_host}, raw=early)
    v = ar.view("dst")
    assert np.array_equal(ar.poison_of("dst", "canary").numpy(), early.numpy()[v.offset:v.end])
    assert (ar.poison_of("src", "nan").numpy().view(np.uint32) == A.NAN_BITS).all()
    assert ar.bytes_of("src").data_ptr() == src.data_ptr() and ar.bytes_of("src").numel() == 4 * N


def test_band_rule_and_arena_size():
    tex = ((6, 64, 256, 4), np.float32)
    assert A.band_for(tex) == 2 * 64 * 256 * 16 and A.band_for(((513, 7), np.float32)) == A.MIN_BAND
    ar = A.Arena(A.arena_bytes(A.band_for(tex), tex), band=A.MIN_BAND, device="cpu")
    with pytest.raises(A.ArenaError, match="too small"):
        ar.output((1 << 20,), np.float32)
    ar2 = A.Arena(A.arena_bytes(A.band_for(tex), tex), band=A.MIN_BAND, device="cpu")
    ar2.output(*tex, name="tex0")
    with pytest.raises(AssertionError, match="band 65536 is below"):
        ar2.check({"tex0": np.zeros(tex[0], np.float32)})


def test_out_arguments_of_the_wrappers_are_checked_before_any_pointer_is_taken(pkg):
    """out= / aux_out=: a tensor that is not on the device, not contiguous, of another type or of another size is refused with
    a TypeError, like an input through _dev_ptr (no device is needed to be refused)."""
    import importlib
    import torch
    PM = importlib.import_module("sdf-viewer_amd.program")
    prm = pkg.default_params()
    pts = torch.zeros((5, 3))
    prog = PM.Program().sphere(0.5).build()
    calls = [lambda o: pkg.sample_points(prm, pts, out=o), lambda o: pkg.normal_points(prm, pts, out=o),
             lambda o: pkg.source_sample_scalar(prm, pts, out=o), lambda o: pkg.source_sample_normal(prm, pts, out=o),
             lambda o: pkg.lattice_points((-1, -1, -1, 1, 1, 1), 2, n=5, out=o),
             lambda o: prog.sample_points(pts, out=o), lambda o: prog.normal_points(pts, out=o)]
    for call in calls:
        for bad in (torch.zeros((5, 7)), torch.zeros((5, 7), dtype=torch.float64), "no tensor"):
            with pytest.raises(TypeError, match="out must be a contiguous float32"):
                call(bad)
    with pytest.raises(TypeError, match="must be a contiguous float32 CUDA"):
        pkg._out_tensor(torch.zeros((4, 7)), (5, 7), torch.float32, "cuda", "out")
