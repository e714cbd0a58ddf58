"""DGCNN classifier on a TensorField (counterpart of the reference's co3d_3d/src/models/mink/dgcnn.py:41-124): four layers
that each rebuild the k-nearest-neighbour graph of every sample in the feature space of their input and run an edge
convolution over it (1x1 convolution of [x_j - x_i ; x_i], batch norm over all edges, LeakyReLU(0.2), maximum over the k
edges); the four outputs concatenated, a per-point linear layer to `emb_dims`, global max and average per sample, and a
three-layer head.  The graph and the edge convolution are the kernels of csrc/graph.hip (minkowski/graph.py): no distance
matrix and no edge-sized tensor is formed.

The samples are the field's batch row ranges, so point counts may differ between samples (the reference's dense [B, C, N]
layout needs them equal); the first layer takes 2 * in_channel inputs (the reference hard-codes 6).  The parameter modules are
the reference's (nn.Conv2d / nn.Conv1d / nn.BatchNorm* / nn.Linear under the same names), so `state_dict()` has exactly its
keys and shapes and the initialisation is torch's; only the forward differs.  The widths after batch norm and the pooled
width (`emb_dims`, `head`) must be multiples of 4, as for the batch-norm and pooling kernels everywhere else."""
import torch
import torch.nn as nn

from nerf_downstream_amd import gin_lite as gin

from .base_model import MinkowskiBaseModel


@gin.configurable
class DGCNN_cls(MinkowskiBaseModel):
    def __init__(self, in_channel, out_channel, k=20, emb_dims=1024, dropout=0.5, channels=(64, 64, 128, 256), head=(512, 256),
                 ME=None):
        super().__init__(3, ME=ME)
        if not hasattr(self._ME, "graph"):
            raise NotImplementedError("DGCNN_cls runs on the HIP backend only (minkowski/graph.py)")
        assert len(channels) == 4 and len(head) == 2
        self.k, self.emb_dims, self.dropout = int(k), emb_dims, dropout
        cin = in_channel
        for i, c in enumerate(channels, start=1):
            setattr(self, f"conv{i}", nn.Sequential(nn.Conv2d(2 * cin, c, kernel_size=1, bias=False), nn.BatchNorm2d(c),
                                                    nn.LeakyReLU(negative_slope=0.2)))
            cin = c
        self.conv5 = nn.Sequential(nn.Conv1d(sum(channels), emb_dims, kernel_size=1, bias=False), nn.BatchNorm1d(emb_dims),
                                   nn.LeakyReLU(negative_slope=0.2))
        self.linear1 = nn.Linear(emb_dims * 2, head[0], bias=False)
        self.bn6 = nn.BatchNorm1d(head[0])
        self.dp1 = nn.Dropout(p=dropout)
        self.linear2 = nn.Linear(head[0], head[1])
        self.bn7 = nn.BatchNorm1d(head[1])
        self.dp2 = nn.Dropout(p=dropout)
        self.linear3 = nn.Linear(head[1], out_channel)
        self.knn_indices = []  # the neighbour tables of the last forward: four int32 [n, k] tensors of global rows

    def _bn_lrelu(self, F, bn):
        ME = self._ME
        training = bn.training or not bn.track_running_stats
        if training and bn.track_running_stats:
            bn.num_batches_tracked += 1
        momentum = bn.momentum if bn.momentum is not None else 1.0 / max(float(bn.num_batches_tracked), 1.0)
        F = ME.norm.BatchNormFunction.apply(F, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, momentum, bn.eps, None, False)
        return ME.eltwise.ActivationFunction.apply(F, "leaky_relu", 0.2, None)

    def forward(self, x):
        pool, G = self._ME.pool, self._ME.graph
        x._settle()
        m = x.coordinate_manager
        boff = m.field_batch_offsets(x.C)
        G.check_sample_sizes(m.field_sample_sizes(x.C), self.k)  # (once per field: the counts came with the offsets' status word)
        F = x.F.float()
        self.knn_indices, outs = [], []
        for conv in (self.conv1, self.conv2, self.conv3, self.conv4):
            idx = G.knn(F, boff, self.k)
            self.knn_indices.append(idx)
            F = G.edge_conv(F, conv[0].weight, conv[1], idx)
            outs.append(F)
        F = torch.cat(outs, 1).mm(self.conv5[0].weight.view(self.emb_dims, -1).t())
        F = self._bn_lrelu(F, self.conv5[1])
        h = torch.cat([pool.GlobalMaxPoolFunction.apply(F, boff)[0], pool.GlobalAvgPoolFunction.apply(F, boff)], 1)
        h = self.dp1(self._bn_lrelu(self.linear1(h), self.bn6))
        h = self.dp2(self._bn_lrelu(self.linear2(h), self.bn7))
        return self.linear3(h)
