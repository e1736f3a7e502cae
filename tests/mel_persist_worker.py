"""Child process of tests/test_gpu_mel_exact.py::test_persistent_form.  pa_mel_frontend_fwd reads PA_MEL_PERSIST once per process, so the
persistent form (resident workgroups walking tiles of 8 frames, the next tile's span prefetched by LDS-DMA) needs a process of its own:
this one runs the fixed-length forward checkers of tests/mel_cases.py on it -- the short clips, both staging forms, and a batch sized
from the device's CU count so that there are more tiles than resident workgroups and a workgroup's second tile lies in another clip."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    assert os.environ.get("PA_MEL_PERSIST") == "1", "start me with PA_MEL_PERSIST=1"
    from tests import mel_cases as M
    from tests.test_gpu_mel_exact import Hip, record
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    hip, n = Hip(), 0
    for c in M.persist_cases(cus):
        paths = M.fwd_paths(c.mp.hop, c.L, fr=M.FR_PERSIST, persist=True)
        M.check_forward(hip, c, lambda group, **figs: record("persist." + group, **figs))
        print(f"{c.name}: B = {c.B}, T = {c.T}, staging {sorted(paths)}: ok", flush=True)
        n += 1
    print(f"mel persist OK: {n} cases on {cus} CUs")


if __name__ == "__main__":
    main()
