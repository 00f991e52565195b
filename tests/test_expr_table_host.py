"""Select trees over a table, host side (no GPU): the library exports the two table entry points and native.py binds them with the
argument lists of their single-segment forms."""
import ctypes


def test_the_table_tree_entry_points_are_exported_and_bound():
    from immutable3_amd import native
    L = native.load()
    for name, seg_form in (("imm3_query_create_table_expr", "imm3_query_create_expr"),
                           ("imm3_query_create_table_agg_expr", "imm3_query_create_agg_expr")):
        assert name in native.EXPORTS
        fn = getattr(L, name)                       # (AttributeError: the symbol is not in the library)
        assert fn.restype is ctypes.c_int
        assert fn.argtypes is not None and list(fn.argtypes) == list(getattr(L, seg_form).argtypes)
        assert len(fn.argtypes) == {"imm3_query_create_table_expr": 13, "imm3_query_create_table_agg_expr": 14}[name]


def test_a_null_table_is_refused_without_a_device():
    from immutable3_amd import native
    L = native.load()
    out = ctypes.c_void_p()
    rc = L.imm3_query_create_table_expr(None, None, None, 0, None, 0, None, 0, None, 0, 0, 1024, ctypes.byref(out))
    assert rc == native.ERR_ARG and b"table is null" in L.imm3_last_error()
    rc = L.imm3_query_create_table_agg_expr(None, None, None, 0, None, 0, None, 0, None, 0, None, 0, 1024, ctypes.byref(out))
    assert rc == native.ERR_ARG and b"table is null" in L.imm3_last_error()
