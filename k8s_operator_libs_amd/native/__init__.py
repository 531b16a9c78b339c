"""Native HIP/gfx950 components (built in-tree via build.py)."""

import os


def load_wire():
    """The native HTTP/1.1 wire extension (``_wire``), or None when it is
    not built or ``K8S_OPERATOR_LIBS_NATIVE_WIRE=0`` disables it.  Same
    pattern as ``meta.deep_copy``: the pure-Python path stays as the
    fallback.  Read at each call, so a client or server picks the switch up
    when it is constructed."""
    if os.environ.get("K8S_OPERATOR_LIBS_NATIVE_WIRE", "1") == "0":
        return None
    try:
        from . import _wire
    except ImportError:
        return None
    return _wire
