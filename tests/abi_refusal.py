"""Helper of the CPU ABI tests: a refused C call must return its code AND name its entry point in mtmc_mpn_last_error().

Before every call under test another entry point (mtmc_pool_tracklets with n_rows = -1, refused before any HIP call) leaves
ITS text in the thread's error buffer, so an exit that writes no text of its own cannot pass for a named one."""
from mtmc_mpn import _lib


def refused(lib, call, code, entry):
    """`call()` returns `code` and the error text starts with "<entry>: " (the name without the mtmc_ prefix)."""
    assert lib.mtmc_pool_tracklets(None, 0, -1, 4, None, 0, None, None, None, 0, None) == _lib.E_ARG
    assert lib.mtmc_mpn_last_error().startswith(b"pool_tracklets: ")
    rc = call()
    text = lib.mtmc_mpn_last_error()
    return rc == code and text.startswith(entry.encode() + b": ")
