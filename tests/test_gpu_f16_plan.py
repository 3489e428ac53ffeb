"""The fp16 launch table a live context runs is the one yolo2_hip_f16_plan_describe prints for the same options (the selection is a
function of the options, the split mode and the batch alone: tests/test_host_logic.py checks its content without a GPU)."""
import pytest

from yolo2_amd import hipdrv, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("split", [0, 1], ids=["fp16", "split"])
def test_live_table_names_the_kernels_describe_names(split):
    model = synth.SynthModel(seed=1)
    ctx = hipdrv.Yolo2Hip(0)
    try:
        ctx.load_weights_fp32(model.weights_f32(), model.bias_f32())
        (ctx.run_batch_f32tol_host if split else ctx.run_batch_fp16_host)(synth.frames(11, 2))
        live = {i: k for i in range(32) if (k := ctx.f32tol_layer_kernel(i))} if split else ctx.fp16_layer_kernels()
        options = ctx.options()
    finally:
        ctx.close()
    want = {}
    for line in hipdrv.f16_plan_describe(options, split, 2).splitlines():
        if line.startswith("L"):
            want.setdefault(int(line.split()[0][1:]), line.split()[1])
    assert len(want) >= 20 and live == want
