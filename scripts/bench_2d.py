"""BASELINE config #5 on the GPU box: the dense 2-D comparison network (ResNet18, 224^2 synthetic renders, batch 32,
LitModel recipe: CE + weight-decay term + SGD) -- images/s forward+backward+update with the convolutions on the bf16
matrix cores and in exact fp32, beside the same network on torch's own dense operators (MIOpen) for orientation.
usage: python scripts/bench_2d.py [batch] [steps] [--model NAME]
--model: one of the Bottleneck networks (resnet50, resnext50_32x4d, ...) instead of resnet18; the torch network beside it is the
plain-torch Bottleneck network of tests/test_gpu_bottleneck2d.py."""
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch
from nerf_downstream_amd.co3d_2d.src.modules.classification import LitModel
from nerf_downstream_amd.minkowski import functional as Fn

argv = list(sys.argv[1:])
MODEL = "resnet18"
if "--model" in argv:
    i = argv.index("--model")
    MODEL = argv[i + 1]
    del argv[i:i + 2]
B = int(argv[0]) if len(argv) > 0 else 32
steps = int(argv[1]) if len(argv) > 1 else 20
dev = torch.device("cuda", 0)
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)
y = torch.randint(0, 51, (B,), device=dev)


def bench(model, opt, step_fn, tag):
    for _ in range(5):
        step_fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step_fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    print(f"{tag}: {ms:.2f} ms/step, {B / ms * 1e3:.0f} images/s")


lit = LitModel(MODEL).to(dev)
opt = lit.configure_optimizers()


def hip_step():
    opt.zero_grad(set_to_none=True)
    loss, _ = lit.training_step({"images": x, "labels": y})
    loss.backward()
    opt.step()


# (the second 25-step window of a fresh process runs 30-100 % slower than the ones before and after it, whatever the math mode -- allocator /
#  clock settling, not the kernels: 8.8 / 11.5 / 8.9 ms in fp32 -- so the process is warmed past it before anything is timed)
for _ in range(60):
    hip_step()
for math in ("bf16", "fp32"):
    Fn.set_conv_math(math)
    bench(lit, opt, hip_step, f"HIP sparse-kernel {MODEL} B={B} 224^2, conv math {math}")
Fn.set_conv_math("fp32")

if MODEL == "resnet18":
    from test_gpu_dense2d import _TorchResNet18
    ref = _TorchResNet18()
else:
    from test_gpu_bottleneck2d import _TorchNet
    from nerf_downstream_amd.co3d_2d.src.model.models import _BOTTLENECK
    ref = _TorchNet(*_BOTTLENECK[MODEL])
ref = ref.to(dev).to(memory_format=torch.channels_last)
ropt = torch.optim.SGD(ref.parameters(), 0.1, momentum=0.9)
xr = x.to(memory_format=torch.channels_last)


def torch_step(amp):
    def f():
        ropt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            loss = torch.nn.functional.cross_entropy(ref(xr), y, label_smoothing=0.005)
        loss.backward()
        ropt.step()
    return f


bench(ref, ropt, torch_step(True), f"torch (MIOpen) {MODEL} channels_last, bf16 autocast")
bench(ref, ropt, torch_step(False), f"torch (MIOpen) {MODEL} channels_last, fp32")
