"""The device MX entry points (csrc/k_mx.hip) without a GPU: exported, and every argument the host entries
reject is rejected on the host before anything is launched (dummy non-null integer pointers, no device)."""
from vsiquantization_amd import _hip as H


def test_device_entries_are_exported_and_check_their_arguments_before_any_launch():
    lib = H.lib()
    for name in ("vsiq_mx_fq_fwd_f32", "vsiq_mx_fq_fwd_cols_f32"):
        assert name in H.EXPORTED and hasattr(lib, name), name
    rows, cols = lib.vsiq_mx_fq_fwd_f32, lib.vsiq_mx_fq_fwd_cols_f32
    for fmt, r, n in ((5, 2, 32), (-1, 2, 32), (0, 0, 32), (0, 2, 0)):   # unknown format, sizes
        assert rows(16, 32, None, None, None, r, n, fmt, None) == -1
        assert cols(16, 32, None, None, None, r, 2, n, fmt, None) == -1
    assert cols(16, 32, None, None, None, 1, 0, 32, 0, None) == -1
    assert rows(None, 32, None, None, None, 2, 32, 0, None) == -1     # no x
    assert cols(None, 32, None, None, None, 1, 2, 32, 0, None) == -1
    for out in range(3):                                              # codes / scales / mask without y
        args = [None, None, None]
        args[out] = 48
        assert rows(16, None, *args, 2, 32, 0, None) == -1
        assert cols(16, None, *args, 1, 2, 32, 0, None) == -1
    assert rows(16, 32, None, None, None, 1 << 40, 1 << 40, 0, None) == -1   # rows * rowlen overflows
    assert rows(16, 32, None, None, None, 1 << 31, 256, 0, None) == -1       # 2^31 chunks of 256
    assert cols(16, 32, None, None, None, 1 << 31, 32, 256, 0, None) == -1   # 2^31 wave tasks
    assert rows(16, 32, None, None, 12, 2, 32, 0, None) == -2                # mask not 8-byte aligned
    assert cols(16, 32, None, None, 12, 1, 2, 32, 0, None) == -2
