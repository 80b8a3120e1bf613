"""The reproducible mode: same inputs, same model / optimizer / generator state, same environment switches -> the same bits
in every output and every gradient, run after run (INTEGRATION section X holds the contract and the audit behind it).

Every float sum of the package has a stated order except three, and the switch settles those three at once:

* the rasterizer's backward stores the row of every (list entry, quadrant) and adds the rows in a fixed order instead of
  with float atomics (what ``GFT_BWD_DETERMINISTIC`` / ``api._DETERMINISTIC`` select for the rasterizer alone);
* the flow renderer's backward (``flow.render_flows`` / ``render_flow_pair``) does the same (``gft_render_features_backward_det``);
* ``DeformNetwork`` chooses its backward route without asking whether a posted row count has reached the host yet
  (``deform._choose_route``): eagerly ``device_row_count == "auto"`` behaves as ``"capture"``.

The switch is read by every call, never baked in at import: a backward runs in the mode that is on when it is launched, and
a captured graph keeps the mode it was captured under.  ``GFT_REPRODUCIBLE=1`` in the environment turns it on at import.
Off (the default) nothing changes anywhere.

``GFT_DET_REDUCE`` (``grid``, the default, or ``serial``) picks how the stored rows are added: across the chip
(``csrc/k_detsum.hip``) or by the one-workgroup comparator; both give the same bits.
"""
import contextlib
import os
import sys
import types

_enabled = os.environ.get("GFT_REPRODUCIBLE", "0") not in ("", "0")
# how the fixed-order modes add their stored rows: "grid" (csrc/k_detsum.hip) or "serial" (the one-workgroup comparator)
_det_reduce = "serial" if os.environ.get("GFT_DET_REDUCE", "grid") == "serial" else "grid"


def set_reproducible(flag):
    """Turns the mode on or off for every later call."""
    global _enabled
    _enabled = bool(flag)


def is_reproducible():
    return _enabled


@contextlib.contextmanager
def reproducible(flag=True):
    """``with reproducible(): ...``: the mode is `flag` inside and what it was before afterwards (also after an exception).
    Nests."""
    global _enabled
    before = _enabled
    _enabled = bool(flag)
    try:
        yield
    finally:
        _enabled = before


def det_reduce():
    """``"grid"`` or ``"serial"``: the sum the fixed-order modes use (an internal switch: the serial one is the comparator)."""
    return _det_reduce


class _CallableModule(types.ModuleType):
    """``gftorf_amd.reproducible`` names this module and, re-exported from the package, its context manager: calling the
    module is calling ``reproducible(flag)``, so both readings of the name work."""

    def __call__(self, flag=True):
        return reproducible(flag)


sys.modules[__name__].__class__ = _CallableModule
