"""Every AdamW entry of the library against the exact model of tests/adamw_cases.py, bit for bit, on the guarded case of
tests/test_gpu_finetune.py (12 397 live elements: a 100 x 70 matrix with copies whose 64-tile has edges both ways, a 4097-element
run, the misaligned 527 / 768 pair, a 5-element vector -- every path of the flat and of the table kernel: aligned and scalar, tile
edge, run tail, transposed copy).  No tolerance, no element left out: parameters and both moments equal the model on the live
elements, both copies equal the updated matrix cast and transposed, every sentinel around them is intact and the gradients are
unwritten.  The hyper-parameters reach the kernels by value and from the device row; the model takes the row pa_adamw_hyper wrote."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib, ops  # noqa: E402
from tests import adamw_cases as AC  # noqa: E402

DEV = "cuda"
BY_VALUE = tuple(AC.HYPER[k] for k in ("lr", "b1", "b2", "eps", "wd", "step"))
# entry -> (takes a table, writes copies, takes scales: "no" / "must" / "may", takes the clip factor, hyper-parameters by value / row)
ENTRIES = {
    "pa_adamw": (False, False, "no", False, (True,)),
    "pa_adamw_dev": (False, False, "no", False, (False,)),
    "pa_adamw_clip": (False, False, "no", True, (True, False)),
    "pa_adamw_stage": (True, True, "no", False, (True, False)),
    "pa_adamw_stage_groups": (True, True, "must", False, (True, False)),
    "pa_adamw_groups": (True, False, "must", False, (True, False)),
    "pa_adamw_stage_clip": (True, True, "may", True, (True, False)),
}


def _launch_and_check(entry, dtype, by_value, which, factor):
    table, copies, _, clips, _ = ENTRIES[entry]
    c = AC.group_case(dtype, DEV)
    dev = {k: c[k].to(DEV) for k in "pgmv"}
    g_before = dev["g"].clone()
    row = AC.hyper_row().to(DEV)
    assert torch.equal(AC.bits(row.cpu()), AC.bits(AC.hyper_row()))        # the row the model was given is the one on the device
    kw = dict(entry=entry)
    if clips and factor is not None:
        kw["gscale"] = torch.tensor([factor], dtype=torch.float32, device=DEV)
    hyper = BY_VALUE if by_value else row
    if table:
        entries = [(off, rows, cols, c["dst"] if cp and copies else None, c["dst_t"] if cp and copies else None)
                   for off, (rows, cols, cp, _) in zip(c["offs"], AC.PARAMS)]
        scales = None if which is None else ops.make_adamw_scales(AC.SCALES[which], DEV)
        ops.adamw_update(dev["p"], dev["g"], dev["m"], dev["v"], hyper, table=ops.make_adamw_stage_table(entries, DEV), scales=scales,
                         dtype=dtype, **kw)
    else:
        for off, (rows, cols, _, _) in zip(c["offs"], AC.PARAMS):          # every parameter as its own flat span (two are misaligned)
            ops.adamw_update(*(dev[k][off:off + rows * cols] for k in "pgmv"), hyper, **kw)
    torch.cuda.synchronize()
    want = AC.expected(which, factor)
    tag = (entry, dtype, by_value, which, factor)
    for k in "pmv":                 # the live elements AND the sentinels between them
        assert torch.equal(AC.bits(dev[k].cpu()), AC.bits(want[k])), (k,) + tag
    assert torch.equal(AC.bits(dev["g"]), AC.bits(g_before)), tag
    cp = AC.expected_copies(want["p"], c, dtype) if copies else torch.full_like(c["copies"], AC.SENT, device="cpu")
    assert torch.equal(AC.bits(c["copies"].cpu()), AC.bits(cp)), tag


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_adamw_entry_equals_the_model_bit_for_bit(entry):
    table, _, scales, clips, modes = ENTRIES[entry]
    for dtype in ((_lib.PA_BF16, _lib.PA_F32) if table else (_lib.PA_F32,)):
        for by_value in modes:
            for which in {"no": (None,), "must": ("a", "b"), "may": (None, "a", "b")}[scales]:
                for factor in (AC.FACTORS if clips else (None,)):
                    _launch_and_check(entry, dtype, by_value, which, factor)
