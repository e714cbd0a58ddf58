"""Writes tests/golden/resunet_state_keys_v1.json: the state-dict names, shapes and order of ResUNetBN2C and ResUNetIN2C at
(in_channel 3, out_channel 32), spelled out from the constructor of the reference's co3d_3d/src/models/mink/resunet.py
(CHANNELS [-, 32, 64, 128, 256], TR_CHANNELS [-, 64, 64, 64, 128]) without importing any model code.

  convolution k=3         : kernel [27, Cin, Cout];  1x1x1 stride 1: kernel [Cin, Cout];  `final` adds bias [1, Cout]
  MinkowskiBatchNorm      : bn.weight, bn.bias, bn.running_mean, bn.running_var [C], bn.num_batches_tracked []
  MinkowskiInstanceNorm   : weight, bias [1, C]
  BasicBlock(c, c)        : conv1, norm1, conv2, norm2 (no downsample)"""
import json
import os

CH, TR = [None, 32, 64, 128, 256], [None, 64, 64, 64, 128]


def norm(prefix, kind, c):
    if kind == "BN":
        return [(f"{prefix}.bn.weight", [c]), (f"{prefix}.bn.bias", [c]), (f"{prefix}.bn.running_mean", [c]),
                (f"{prefix}.bn.running_var", [c]), (f"{prefix}.bn.num_batches_tracked", [])]
    return [(f"{prefix}.weight", [1, c]), (f"{prefix}.bias", [1, c])]


def stage(conv, nrm, block, cin, cout, block_norm):
    out = [(f"{conv}.kernel", [27, cin, cout])] + norm(nrm, "BN", cout)
    for i in (1, 2):
        out += [(f"{block}.conv{i}.kernel", [27, cout, cout])] + norm(f"{block}.norm{i}", block_norm, cout)
    return out


def keys(block_norm, cin=3, cout=32):
    out = stage("conv1", "norm1", "block1", cin, CH[1], block_norm)
    out += stage("conv2", "norm2", "block2", CH[1], CH[2], block_norm)
    out += stage("conv3", "norm3", "block3", CH[2], CH[3], block_norm)
    out += stage("conv4", "norm4", "block4", CH[3], CH[4], block_norm)
    out += stage("conv4_tr", "norm4_tr", "block4_tr", CH[4], TR[4], block_norm)
    out += stage("conv3_tr", "norm3_tr", "block3_tr", CH[3] + TR[4], TR[3], block_norm)
    out += stage("conv2_tr", "norm2_tr", "block2_tr", CH[2] + TR[3], TR[2], block_norm)
    out += [("conv1_tr.kernel", [CH[1] + TR[2], TR[1]]), ("final.kernel", [TR[1], cout]), ("final.bias", [1, cout])]
    return [[k, s] for k, s in out]


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "resunet_state_keys_v1.json")
    with open(path, "w") as f:
        json.dump({"in_channel": 3, "out_channel": 32, "ResUNetBN2C": keys("BN"), "ResUNetIN2C": keys("IN")}, f, indent=0)
        f.write("\n")
    print(path)
