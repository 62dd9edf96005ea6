"""What the ABI tests of the three re-projection layers (tests/test_abi_projection.py, test_abi_dense_projection.py,
test_abi_reverse_projection.py) share: a valid parameter struct with a host buffer that stands in for every device
pointer, a call with some arguments replaced, and the out-of-range rows of the parameters the layers have in common."""
import ctypes as C

NULL, RANGE, TYPE, WORKSPACE, CAMERA = -1, -2, -3, -4, -5        # SRH_E_*
BIG = 1 << 40

# (field, value, code): the batch, the frame and the channels, which every layer has; the pinhole of the one-camera layers
FRAME_ROWS = [("n_views", 0, RANGE), ("n_views", 65536, RANGE), ("width", 0, RANGE), ("height", 0, RANGE),
              ("width", 1 << 22, RANGE), ("channels", 0, RANGE), ("channels", 5, RANGE)]
PINHOLE_ROWS = [("fovy", 0.0, CAMERA), ("fovy", 3.2, CAMERA), ("fovy", float("nan"), CAMERA),
                ("focal_length", 0.0, CAMERA), ("focal_length", float("inf"), CAMERA)]


def valid_params(struct, **fields):
    """(params, the address every pointer argument gets, the buffer behind it)."""
    buf = (C.c_double * 64)()
    return struct(**fields), C.addressof(buf), buf


def pointers(arg_spec):
    return [k for k in arg_spec if not k.endswith("_bytes")]


def call(fn, arg_spec, p, a, **given):
    """fn(params, *arg_spec, stream = NULL): a pointer argument is `a` and a `*_bytes` argument BIG, unless `given` names
    it (None: a NULL pointer)."""
    return fn(C.byref(p), *[given.get(k, BIG if k.endswith("_bytes") else a) for k in arg_spec], None)


def assert_refused_by_name(lib, calls, workspace_bytes, p, a, field, code):
    """Every entry point among `calls` returns `code` and names the field; the size function answers 0."""
    name = {"width": b"width x height", "height": b"width x height"}.get(field, field.encode())
    for c in calls:
        assert c(lib, p, a) == code, c.__name__
        assert name in lib.srh_last_error(), (c.__name__, lib.srh_last_error())
    assert workspace_bytes(C.byref(p), 0) == 0
