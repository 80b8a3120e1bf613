"""deform._choose_route: the route of a DeformNetwork call's backward, chosen once in the forward.  Host only: no device,
no library.  The yardstick is `_earlier_route`, the conditions the forward and the backward evaluated separately before the
routes had names, kept here as they stood."""
import itertools

import pytest

from helpers import deform_modes

DEFAULTS = dict(sparse_backward=True, lazy_save=True, device_row_count="auto")
STATES = (None, "unknown", 0.2, 0.25, 0.5, 0.6, 0.7)


def _state(s):
    return None if s is None else {"fraction": None if s == "unknown" else s}


class _WorkBytes:
    """The size of the rows work buffer as a callable that counts how often it is asked."""

    def __init__(self, value):
        self.value, self.calls = value, 0

    def __call__(self):
        self.calls += 1
        return self.value


def _earlier_route(D, need_bw, n, capturing, state, work_bytes):
    # the forward: what it kept for the backward
    sparse_ok = bool(need_bw and D.sparse_backward and n >= D._SPARSE_MIN_POINTS)
    dev_mode = None
    if sparse_ok and D.device_row_count is not False:
        if D.device_row_count is True or (capturing and D.device_row_count in ("capture", "auto")):
            dev_mode = "rows"
        elif D.device_row_count == "auto" and state is not None and work_bytes() <= D._DEVICE_ROWS_MAX_BYTES:
            frac = state.get("fraction")
            dev_mode = "rows" if (frac is not None and frac <= D._DEVICE_ROWS_MAX_FRACTION and D.lazy_save) else "count"
    dev_rows = dev_mode == "rows"
    lazy = bool(sparse_ok and D.lazy_save and state is not None and dev_mode is None
                and state.get("fraction") is not None and state["fraction"] <= D._LAZY_MAX_FRACTION and not capturing) or dev_rows
    dev_count = dev_mode == "count"
    # the backward: what it did with that (an upstream gradient present)
    if not need_bw:
        return "none"                                   # nothing saved: raises
    if dev_rows:
        return "rows"
    if lazy:
        return "recompute"
    if D.sparse_backward and n >= D._SPARSE_MIN_POINTS and not dev_count and not capturing:
        return "compact"
    return "count" if dev_count else "dense"


def test_every_combination_takes_the_route_the_separate_conditions_gave():
    cases = 0
    for sparse, lazy_save, mode in itertools.product((False, True), (False, True), (False, True, "capture", "auto")):
        with deform_modes(sparse_backward=sparse, lazy_save=lazy_save, device_row_count=mode) as D:
            sizes = (0, D._SPARSE_MIN_POINTS - 1, D._SPARSE_MIN_POINTS)
            buffers = (D._DEVICE_ROWS_MAX_BYTES, D._DEVICE_ROWS_MAX_BYTES + 1)
            for need_bw, n, capturing, s, nbytes in itertools.product((False, True), sizes, (False, True), STATES, buffers):
                want_bytes, got_bytes = _WorkBytes(nbytes), _WorkBytes(nbytes)
                want = _earlier_route(D, need_bw, n, capturing, _state(s), want_bytes)
                got = D._choose_route(need_bw, n, capturing, _state(s), got_bytes)
                case = (sparse, lazy_save, mode, need_bw, n, capturing, s, nbytes)
                assert got == want, case
                assert got == D._choose_route(need_bw, n, capturing, _state(s), nbytes), case      # (the size as a number)
                assert got_bytes.calls == want_bytes.calls <= 1, case
                if not need_bw or capturing or mode != "auto":      # asked under "auto", eagerly, only
                    assert got_bytes.calls == 0, case
                cases += 1
    assert cases == 2688


MIN = "min"         # stands for _SPARSE_MIN_POINTS
SPOT_ROWS = {
    # name: (switches over DEFAULTS, need_bw, n, capturing, state, work buffer too large, route)
    "default_eager_share_unknown": ({}, True, MIN, False, "unknown", False, "count"),
    "default_eager_share_half": ({}, True, MIN, False, 0.5, False, "rows"),
    "default_eager_share_large": ({}, True, MIN, False, 0.7, False, "count"),
    "default_capturing": ({}, True, MIN, True, "unknown", False, "rows"),
    "never_on_device_capturing": (dict(device_row_count=False), True, MIN, True, "unknown", False, "dense"),
    "capture_only_eager_share_small": (dict(device_row_count="capture"), True, MIN, False, 0.2, False, "recompute"),
    "capture_only_eager_share_half": (dict(device_row_count="capture"), True, MIN, False, 0.5, False, "compact"),
    "always_save_auto_share_small": (dict(lazy_save=False), True, MIN, False, 0.2, False, "count"),
    "no_state_auto_eager": ({}, True, MIN, False, None, False, "compact"),
    "work_buffer_too_large": ({}, True, MIN, False, 0.2, True, "recompute"),
    "below_the_minimum": ({}, True, -1, False, 0.2, False, "dense"),
    "no_gradient_wanted": ({}, False, MIN, False, 0.2, False, "none"),
}


@pytest.mark.parametrize("name", sorted(SPOT_ROWS))
def test_named_rows_of_the_route_table(name):
    switches, need_bw, n, capturing, s, too_large, route = SPOT_ROWS[name]
    with deform_modes(**dict(DEFAULTS, **switches)) as D:
        n = D._SPARSE_MIN_POINTS + (0 if n == MIN else n)
        nbytes = D._DEVICE_ROWS_MAX_BYTES + (1 if too_large else 0)
        assert D._choose_route(need_bw, n, capturing, _state(s), nbytes) == route


def test_the_route_table_names_every_route():
    from gftorf_amd import deform as D
    for route in ("none", "dense", "compact", "recompute", "count", "rows"):
        assert '"%s"' % route in D._choose_route.__doc__
    assert sorted(D._SELECT) == ["compact", "count", "dense", "recompute"]
