"""The D1 + E loop of k_fill3 (the passes over a wave's task table: vertex records gathered, distances, logistic
factors, survivors appended) issues its loads ahead of their use: the task words and records of both passes of an
iteration together, and - in the four- and eight-wave builds with one frame per workgroup - those of the NEXT two
passes before the arithmetic of the current two.  Only the order of issue differs from the plain loop, so every launch
shape must give the same rows bit for bit, and the general kernel (SITATOR_FILL_KERNEL=1, the reference's expressions)
the same zero pattern and the same values within the 1e-6 contract.

The sixteen-wave build does not request ahead, the flat form (SITATOR_F3_SLOT=0) cuts the D0 passes differently: both
are compared with the default launch in every case.  Each case says how it knows that it occurred: the work census of
a SITATOR_DEBUG_STOP=9 fill (sit_info [24..27]: tasks that passed D0, candidate tasks, survivors at the list checks,
windows), sit_info [23] (exact redo passes), or arithmetic on the shape and on the rows' lengths."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = ({}, {"SITATOR_FILL_WAVES": "16"}, {"SITATOR_F3_SLOT": "0"}, {"SITATOR_FILL_WAVES": "8"})


def _with_env(env, fn):
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _contexts(cfg, M, F, seed, mutate=None):
    """The third-generation context and the general kernel's rows of the same trajectory."""
    from sitator_amd import synth
    from tests.test_gpu_kernels import _setup
    host = synth.config_host(cfg)
    ctx, *_ = _setup(host, M, F, seed=seed, kernel="3", mutate=mutate)
    gen, *_ = _setup(host, M, F, seed=seed, kernel="1", mutate=mutate)
    assert gen.fill(check_for_zeros=False)[0] == 0 and gen.info()["fill_kernel"] == 1
    vmax = max(len(v) for v in host.vertices)
    vp = 4
    while vp < vmax:
        vp *= 2
    return ctx, gen.rows_dense(), 64 // vp


def _fill(ctx, env):
    def run():
        rc, nz, err = ctx.fill(check_for_zeros=False)
        assert rc == 0
        info = ctx.info()
        assert info["fill_kernel"] == 3
        return ctx.rows_dense(), info
    return _with_env(env, run)


def _census(ctx, env):
    """tasks that passed D0, candidate tasks, survivors summed over the list checks, windows - of the same launch shape
    (the census build takes the flat form; the tasks of a window are the same in either form)"""
    e = dict(env)
    e["SITATOR_DEBUG_STOP"] = "9"
    return _fill(ctx, e)[1]["census"]


def _agree(ctx, general, env, shapes=SHAPES):
    """Rows under `env` in every launch shape: equal bit for bit, and the general kernel's within the contract."""
    base, info0 = _fill(ctx, env)
    assert np.array_equal(base != 0, general != 0), "zero pattern differs from the general kernel's"
    np.testing.assert_allclose(base, general, rtol=1e-6, atol=0)
    for shape in shapes[1:]:
        e = dict(env)
        e.update(shape)
        got, info = _fill(ctx, e)
        if "SITATOR_FILL_WAVES" in shape:
            assert info["waves_per_workgroup"] == int(shape["SITATOR_FILL_WAVES"])
        if shape.get("SITATOR_F3_SLOT") == "0":
            assert info["fill_slot_width"] == 0
        assert np.array_equal(base, got), shape
    return base, info0


def _window_survivors(rows, M, iw):
    """survivors of every window: the non-zero entries of its ions' rows (frame-major rows, windows of iw ions of a frame)"""
    nnz = (rows != 0).sum(axis=1).reshape(-1, M)
    return np.array([[nnz[f, a:a + iw].sum() for a in range(0, M, iw)] for f in range(nnz.shape[0])])


def test_tables_that_drain_in_one_pass_in_an_odd_and_in_an_even_number_of_passes():
    """One window per frame (IW = M, one frame per workgroup), every frame a copy of the first, a task table that holds
    the whole window: the census' tasks per window are then THE number of tasks of every window of the launch, and
    ceil(tasks / tasks per pass) its passes - one pass (a single-pass body and nothing requested ahead), an odd number
    (two-pass bodies, requests ahead, a single pass at the end) and an even number (the last request ahead is skipped).
    All three must occur among the launches."""
    seen = {}
    for cfg, M, seed in (("C2", 1, 71), ("C2", 2, 73), ("C5", 1, 79), ("C2", 4, 3), ("C2", 8, 5), ("C2", 12, 7), ("C2", 16, 11), ("C2", 20, 13), ("C2", 32, 17), ("C2", 48, 19),
                         ("C2", 64, 23), ("C5", 4, 29), ("C5", 8, 31), ("C5", 16, 37), ("C5", 24, 41), ("C5", 40, 43)):
        def copies(frames, sm, mm):
            frames[:] = frames[0]
        ctx, general, tpp = _contexts(cfg, M, 6, seed, mutate=copies)
        env = {"SITATOR_FILL_IW": str(max(M, 4)), "SITATOR_FILL_FPB": "1", "SITATOR_FILL_WAVES": "4", "SITATOR_FILL_TCAP": "512"}
        tasks, cand, surv, windows = _census(ctx, env)
        assert windows == 6, "one window per frame"
        assert tasks % 6 == 0 and tasks / 6 <= 512 - 64, "every window the same, drained once"
        passes = -(-int(tasks / 6) // tpp)
        kind = "none" if passes == 0 else "one" if passes == 1 else "odd" if passes % 2 else "even"
        seen.setdefault(kind, []).append((cfg, M, passes))
        print("%s M %d: %d tasks per window, %d passes (%s)" % (cfg, M, tasks / 6, passes, kind))
        _agree(ctx, general, env, shapes=({}, {"SITATOR_F3_SLOT": "0"}, {"SITATOR_FILL_TCAP": "128"}))
    assert {"one", "odd", "even"} <= set(seen), seen


@pytest.mark.parametrize("cfg,M,F", [("C2", 64, 90), ("C5", 160, 30)])
@pytest.mark.parametrize("iw", ["4", "8", "16", "32", "64"])
def test_window_sizes_agree(cfg, M, F, iw):
    """Windows of 4 to 64 ions: tables of a few tasks up to tables that fill and drain in mid-window (the census gives the
    mean number of tasks per window: 9 to 150 at C2, 22 to 350 at C5, eight to a pass); the windows of every frame differ,
    so passes of every count and parity are mixed here - the launches with ONE known count are the test above."""
    ctx, general, tpp = _contexts(cfg, M, F, seed=47)
    env = {"SITATOR_FILL_IW": iw, "SITATOR_FILL_FPB": "1"}
    tasks, cand, surv, windows = _census(ctx, env)
    assert windows == F * -(-M // int(iw)), "the windows the shape asks for"
    print("%s IW %s: %.1f tasks per window, %d per pass" % (cfg, iw, tasks / windows, tpp))
    _agree(ctx, general, env)


@pytest.mark.parametrize("cfg,M,F", [("C2", 64, 90), ("C5", 160, 30)])
@pytest.mark.parametrize("rcap", ["8", "16", "24"])
def test_survivor_list_that_fills_in_mid_window(cfg, M, F, rcap):
    """Eight tasks per pass: with eight slots a pass fits an EMPTY list only - the single-pass body alone runs, and the
    list leaves for the row buffers (F3_T_ROUND(0)) whenever a pass left survivors and passes remain; with 16 and 24
    slots the two-pass body runs on an empty list and the single-pass body behind it.  That the list does fill: the
    rows say how many survivors a window has, and the first window with more of them than slots must empty its list
    in mid-window."""
    ctx, general, tpp = _contexts(cfg, M, F, seed=53)
    assert tpp == 8
    env = {"SITATOR_FILL_RCAP": rcap, "SITATOR_FILL_FPB": "1"}
    base, info = _agree(ctx, general, env)
    assert info["survivors_per_wave"] == int(rcap)
    # (the window follows from the shape: the frame's ions dealt to the waves, in fours, 16 to 64)
    iw = min(64, max(16, (-(-M // info["waves_per_workgroup"]) + 3) // 4 * 4))
    surv = _window_survivors(base, M, iw)
    print("%s RCAP %s: survivors per window %d .. %d" % (cfg, rcap, surv.min(), surv.max()))
    assert (surv > int(rcap)).any(), "no window outgrows its list: the case did not occur"


def test_task_table_drained_more_than_once_per_window():
    """C5 keeps about six components per ion: a window of 64 ions has several hundred survivors, a table of 64 entries
    holds 64 tasks at most, so every window with more than 64 survivors drained its table more than once."""
    ctx, general, tpp = _contexts("C5", 160, 30, seed=59)
    env = {"SITATOR_FILL_TCAP": "64", "SITATOR_FILL_IW": "64", "SITATOR_FILL_FPB": "1"}
    base, info = _agree(ctx, general, env)
    assert info["task_table_per_wave"] == 64
    surv = _window_survivors(base, 160, 64)
    print("survivors per window %d .. %d" % (surv.min(), surv.max()))
    assert (surv > 64).any(), "no window has more survivors than the table holds"
    # ... and with the survivor list filling at the same time
    env["SITATOR_FILL_RCAP"] = "16"
    _agree(ctx, general, env)


@pytest.mark.parametrize("cfg,M,F", [("C2", 64, 90), ("C5", 160, 30)])
def test_exact_redo_path_is_entered(cfg, M, F):
    """SITATOR_F3_FORCE_EXACT opens the band of the cheap decision: every group of passes goes round again with the
    reference's arithmetic (sit_info [23] counts them) - on the records of the current passes, while those of the next
    are on their way."""
    ctx, general, tpp = _contexts(cfg, M, F, seed=61)
    plain, info = _fill(ctx, {})
    assert info["band_redos"] == 0
    for extra in ({}, {"SITATOR_FILL_RCAP": "16"}, {"SITATOR_FILL_IW": "4", "SITATOR_FILL_FPB": "1"}):
        env = {"SITATOR_F3_FORCE_EXACT": "1"}
        env.update(extra)
        base, info = _agree(ctx, general, env)
        assert info["band_redos"] > 0, "the exact path was not entered"
        assert np.array_equal(base != 0, plain != 0)
        # (the exact pass takes the reference's distance, the plain one the minimum-image distance: the logistic arguments
        # differ by the band's width at most, ~1e-11, a factor by as much relatively, a product of 16 by 16 times that)
        np.testing.assert_allclose(base, plain, rtol=1e-9, atol=0)


@pytest.mark.parametrize("M,iw", [(57, "16"), (57, "12"), (30, "16"), (61, "64")])
def test_last_window_of_a_frame_shorter_than_the_others(M, iw):
    """M is not a multiple of the window: the last window of every frame has M mod IW ions (9, 9, 14 and 61 of 16, 12, 16
    and 64), its passes read task words of lanes beyond its tasks and the request ahead a stale part of the table."""
    assert M % int(iw) != 0
    ctx, general, tpp = _contexts("C2", M, 90, seed=67)
    env = {"SITATOR_FILL_IW": iw, "SITATOR_FILL_FPB": "1"}
    tasks, cand, surv, windows = _census(ctx, env)
    assert windows == 90 * -(-M // int(iw))
    _agree(ctx, general, env)
