"""Record a library build's loss workspace sizes over the table of tests/test_loss_ws_cpu.py -> tests/loss_ws_answers.json (the yardstick
of that test: recorded from the commit BEFORE a change to the workspace layout, compared at the change).  No device is touched.

    BNERV_LIB=/path/to/parent/libbnerv_hip.so python tools/record_loss_ws.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_loss_ws_cpu as T                                  # noqa: E402
from boosting_nerv_amd import _lib as L                       # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "loss_ws_answers.json")
ans = T.answers(L.load())
with open(out, "w") as f:
    json.dump(ans, f, separators=(",", ":"))
    f.write("\n")
print(f"{out}: {len(ans)} answers from {L.LIB_PATH}")
