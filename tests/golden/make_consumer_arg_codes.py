"""Writes tests/golden/consumer_arg_codes.json and consumer_arg_codes_more.json: what the library answers to every call of
tests/test_consumer_args_order.py, each consumer in the file the test's RECORDED names for it.

    TRPX_LIB=/path/to/the/recorded/libtrpx_hip.so python tests/golden/make_consumer_arg_codes.py

Run it with the library of the commit whose behaviour is to be kept, on a machine without a HIP device (the _host forms that
look for the device first then answer NO_DEVICE, which is how the test tells them from the others)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from trpx_amd import _lib                                    # noqa: E402
import test_consumer_args_order as T                         # noqa: E402

L = _lib.lib()
if L.trpx_device_count():
    sys.exit("a HIP device is present: the _host column is recorded without one")
got = T.answers(L)
for path, names in T.RECORDED.items():
    part = T._of(got, names)
    with open(path, "w") as f:
        json.dump(part, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{_lib.LIB_PATH}: {len(part['ptr'])} device-pointer calls, {len(part['host'])} host calls -> {path}")
