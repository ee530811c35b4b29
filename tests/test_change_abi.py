"""The change layer's C-ABI (include/vina_gpu.h "Change layer"): the records'
documented sizes, the binding's layouts against the header as a C compiler
sees it, and the six entry points in the library (no compute calls: CPU-only)."""
import ctypes

import vgpu
from test_abi import _c_layout

SYMBOLS = ["vg_change_begin", "vg_change_accumulate", "vg_change_accumulate_dev", "vg_change_report",
           "vg_change_clear", "vg_change_end"]


def test_record_sizes(tmp_path):
    """vg_change_leaf is 112 bytes and vg_change_cell 56, and the numpy record types are those layouts."""
    for struct, dtype, size in (("vg_change_leaf", vgpu.CHANGE_LEAF_DTYPE, 112),
                                ("vg_change_cell", vgpu.CHANGE_CELL_DTYPE, 56)):
        names = list(dtype.names)
        csize, offs = _c_layout(tmp_path, struct, names)
        assert csize == size == dtype.itemsize
        assert [dtype.fields[f][1] for f in names] == offs


def test_ctypes_layouts_match_header(tmp_path):
    for struct, cls in (("vg_change_totals", vgpu.ChangeTotals), ("vg_change_params", vgpu.ChangeParams),
                        ("vg_change_query", vgpu.ChangeQuery)):
        names = [f for f, _ in cls._fields_]
        size, offs = _c_layout(tmp_path, struct, names)
        assert ctypes.sizeof(cls) == size, struct
        assert [getattr(cls, f).offset for f in names] == offs, struct
    assert ctypes.sizeof(vgpu.ChangeTotals) == 128


def test_symbols_exported():
    vgpu.build()
    L = ctypes.CDLL(vgpu.LIB)
    assert all(s in vgpu.header_symbols() for s in SYMBOLS)
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
