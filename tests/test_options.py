"""crt_set_option: every option's accepted values, the nearest values outside them, the names, and that options are speed and
set-up knobs only.  The accepted values are the C ABI's contract (include/crt_hip.h)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, 1
INT_MIN, INT_MAX = -2**31, 2**31 - 1
STACK_ENTRIES = 32       # render_kernels.h kStackEntries
LBVH, PLOC = 0, 1        # bvh_build.h kGpuBuilderLbvh / kGpuBuilderPloc


def _range(lo, hi):
    """lowest and highest accepted value, and the nearest value outside on each side that an int can hold"""
    return (lo, hi), tuple(v for v in (lo - 1, hi + 1) if INT_MIN <= v <= INT_MAX)


# name: (accepted values, nearest values outside, default)
OPTIONS = {
    "gpu_build": (*_range(INT_MIN, INT_MAX), 0),
    "dynamic": (*_range(INT_MIN, INT_MAX), 0),
    "seed": (*_range(INT_MIN, INT_MAX), 1234),
    "gpu_builder": ((LBVH, PLOC), (-1, 2), LBVH),
    "bvh_width": ((0,), (-1, 1, 4, 8), 0),
    "spp": (*_range(1, 65536), 4),
    "max_bounces": (*_range(0, 64), 3),
    "phong_ks": (*_range(0, 100000), 0),
    "phong_exponent": (*_range(1, 65536), 32),
    "path_pipeline": ((0, 1), (-1, 2), 0),
    "path_pass_paths": (*_range(1 << 16, 1 << 25), 1 << 24),
    "path_ranges": ((1, 8), (0, 2, 7, 9), 8),
    "path_tile": ((0, 8, 16), (-1, 1, 4, 7, 9, 15, 17), 0),
    "inner_min": ((-8, -1, 1, 65), (-9, 0, 66), -6),
    "inner_min_any": ((-8, -1, 1, 65), (-9, 0, 66), -6),
    "list_short_max": (*_range(1, 1024), 24),
    "xcd_group": ((1, 2, 4, 8, 16), (0, 3, 5, 7, 9, 15, 17, 32), 16),
    "xcd_affine_order": ((0, 1), (-1, 2), 0),
    "split_units": (*_range(-1, 65536), -1),
    "split_rays": ((4, 8, 16), (2, 3, 5, 7, 9, 15, 17, 32), 4),
    "split_segments": ((4, 8, 16), (2, 3, 5, 7, 9, 15, 17, 32), 16),
    "boost_units": (*_range(0, INT_MAX), 512),
    "remeasure_every": (*_range(1, 1024), 1),
    "adaptive_order": ((0, 1, 2), (-1, 3), 2),
    "stack_entries": (*_range(0, STACK_ENTRIES), 0),
    "wide_offsets": ((0, 1), (-1, 2), 0),
}
# compiled in by the diagnostic builds alone: (accepted there, outside there, default)
DIAGNOSTIC = {
    "debug_skip_units": (*_range(0, INT_MAX), 0),
    "timeline": (*_range(INT_MIN, INT_MAX), 0),
    "debug_force_measure": (*_range(INT_MIN, INT_MAX), 0),
}


def _set(pkg, r, name, value):
    return pkg.lib().crt_set_option(r.h, name.encode(), value)


def _error(pkg, r):
    return pkg.lib().crt_last_error(r.h).decode()


def test_every_option_accepts_its_values_and_refuses_the_nearest_outside(pkg):
    assert STACK_ENTRIES == 32 and OPTIONS["stack_entries"][1] == (-1, 33)
    for name, (accepted, outside, default) in OPTIONS.items():
        r = pkg.Renderer(0)  # one context per option: nothing another option left behind decides an answer
        try:
            for v in accepted:
                assert _set(pkg, r, name, v) == OK, "%s=%d: %s" % (name, v, _error(pkg, r))
            for v in outside:
                assert _set(pkg, r, name, v) == EINVAL, "%s=%d was accepted" % (name, v)
                assert name in _error(pkg, r), "%s=%d: the message does not name the option: %r" % (name, v, _error(pkg, r))
            assert _set(pkg, r, name, default) == OK  # a refusal leaves the option usable
        finally:
            r.close()


def test_unknown_and_null_names_are_refused(pkg):
    r = pkg.Renderer(0)
    try:
        for name in ("no_such_option", "", "SPP", "spp ", "sp"):
            assert _set(pkg, r, name, 1) == EINVAL, name
            assert "unknown option '%s'" % name in _error(pkg, r)
        assert pkg.lib().crt_set_option(r.h, None, 0) == EINVAL
        assert pkg.lib().crt_set_option(None, b"spp", 4) == EINVAL
        assert pkg.lib().crt_set_option(None, None, 0) == EINVAL
    finally:
        r.close()


def test_diagnostic_options_are_accepted_or_named_as_such(pkg):
    for name, (accepted, outside, default) in DIAGNOSTIC.items():
        r = pkg.Renderer(0)
        try:
            answers = [_set(pkg, r, name, v) for v in accepted]
            if answers[0] == OK:  # a diagnostic build
                assert answers == [OK] * len(accepted), name
                for v in outside:
                    assert _set(pkg, r, name, v) == EINVAL and name in _error(pkg, r), "%s=%d" % (name, v)
                assert _set(pkg, r, name, default) == OK
            else:
                assert answers == [EINVAL] * len(accepted), name
                for v in accepted + outside:
                    assert _set(pkg, r, name, v) == EINVAL
                    assert name in _error(pkg, r) and "exists only in the diagnostic build" in _error(pkg, r), _error(pkg, r)
        finally:
            r.close()


def test_options_never_change_results(pkg, scenes):
    """a frame before any option was touched and one after every option went through its values and back to its default"""
    quad = scenes._mesh([(-1.5, -1.0, -3.0), (1.5, -1.0, -3.5), (1.5, 1.0, -3.0), (-1.5, 1.0, -2.5)], [(0, 1, 2), (0, 2, 3)], 0)
    r = pkg.Renderer(0)
    try:
        r.upload([quad], [((0.5, 0.8, 0.0), 60.0)], [{"albedo": (0.9, 0.6, 0.3), "type": 1}])
        r.set_camera((0.0, 0.0, 0.0), scenes.IDENTITY)
        r.change_shading_mode(100)
        before = r.render_frame(64, 36)
        assert (before["hit_prim"] != pkg.MISS).any() and (before["hit_prim"] == pkg.MISS).any()  # surface and background both
        for name, (accepted, _, default) in list(OPTIONS.items()) + list(DIAGNOSTIC.items()):
            answers = [_set(pkg, r, name, v) for v in accepted + (default,)]
            assert name in DIAGNOSTIC or answers == [OK] * len(answers), name
        after = r.render_frame(64, 36)
        arrays = [k for k, v in before.items() if isinstance(v, np.ndarray)]
        assert {"rgba8", "rgb", "hit_inst", "hit_prim", "hit_t"} <= set(arrays)
        for k in arrays:
            assert before[k].dtype == after[k].dtype and before[k].tobytes() == after[k].tobytes(), k
    finally:
        r.close()
