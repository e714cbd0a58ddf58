"""PAConv classifiers on a TensorField whose features are the xyz (counterparts of the reference's
co3d_3d/src/models/paconv/PointNet_PAConv.py:23-139 and DGCNN_PAConv.py:20-177): one k-nearest-neighbour graph per sample in
xyz, shared by every layer; a ScoreNet per layer turns (x_j - x_i, x_j) into M scores per edge, and the layer's output is the
score-weighted sum over the edges of the features transformed by the M matrices of its weight bank.  The graph, the
aggregation and its gradients are the kernels of csrc/graph.hip and csrc/paconv.hip (minkowski/graph.py, minkowski/paconv.py):
the reference's [B, N, M, O] transformed tensors and its atomicAdd kernels have no counterpart here.

The samples are the field's batch row ranges, so point counts may differ between samples.  The parameter modules are the
reference's under the same names, so `state_dict()` has exactly its keys and shapes, and the weight banks `matrice*` keep its
[Cin', M O] layout and its initialisation (kaiming_normal_ on [M, Cin', O], then the permute and view).  `channels`, `emb_dims`
and `head` allow small instances; every width after a batch norm and the pooled width must be a multiple of 4, as for the
batch-norm and pooling kernels everywhere else."""
import torch
import torch.nn as nn

from nerf_downstream_amd import gin_lite as gin

from .base_model import MinkowskiBaseModel


def _bank(m, cin, cout):
    t = nn.init.kaiming_normal_(torch.empty(m, cin, cout), nonlinearity="relu")
    return nn.Parameter(t.permute(1, 0, 2).contiguous().view(cin, m * cout), requires_grad=True)


class _PAConvBase(MinkowskiBaseModel):
    def __init__(self, ME):
        super().__init__(3, ME=ME)
        if not hasattr(self._ME, "paconv"):
            raise NotImplementedError(f"{type(self).__name__} runs on the HIP backend only (minkowski/paconv.py)")
        self.knn_indices = []  # the neighbour table of the last forward: one int32 [n, k] tensor of global rows

    def _graph(self, x):
        """-> (xyz [n, C], batch offsets, idx, the ScoreNet rows [n k, 2 C], the shared incoming-edge lists)"""
        ME = self._ME
        x._settle()
        m = x.coordinate_manager
        boff = m.field_batch_offsets(x.C)
        ME.graph.check_sample_sizes(m.field_sample_sizes(x.C), self.k)
        F = x.F.float()
        idx = ME.graph.knn(F, boff, self.k)  # unlike DGCNN, the search is in xyz only
        self.knn_indices = [idx]
        return F, boff, idx, ME.paconv.scorenet_input(F, idx), ME.field.lazy_index_csr(idx, F.shape[0])

    def _layer(self, i, h, rows, idx, csr, mode, bias):
        P = self._ME.paconv
        scores = getattr(self, f"scorenet{i}")(rows, self.k, calc_scores=self.calc_scores, bias=bias)
        h = P.paconv(h, getattr(self, f"matrice{i}"), scores, idx, mode, csr_fn=csr)
        return P.batch_norm_rows(h, getattr(self, f"bn{i}"), True)


@gin.configurable
class PAConvPointNet(_PAConvBase):
    def __init__(self, in_channel, out_channel, k=20, calc_scores="softmax", num_matrices=(8, 8, 8), dropout=0.5,
                 channels=(64, 64, 64, 128), emb_dims=1024, head=512, ME=None):
        super().__init__(ME)
        ScoreNet = self._ME.paconv.ScoreNet
        assert len(num_matrices) == 3 and len(channels) == 4
        self.k, self.calc_scores = int(k), calc_scores
        self.m2, self.m3, self.m4 = num_matrices
        for i, m in zip((2, 3, 4), num_matrices):
            setattr(self, f"scorenet{i}", ScoreNet(2 * in_channel, m, hidden_unit=[16]))
        for i, m in zip((2, 3, 4), num_matrices):  # convolutional weight matrices in the weight bank
            setattr(self, f"matrice{i}", _bank(m, channels[i - 2], channels[i - 1]))
        for i, c in enumerate(channels, start=1):
            setattr(self, f"bn{i}", nn.BatchNorm1d(c))
        self.bn5 = nn.BatchNorm1d(emb_dims)
        self.conv1 = nn.Conv1d(in_channel, channels[0], kernel_size=1, bias=False)
        self.conv5 = nn.Conv1d(channels[3], emb_dims, kernel_size=1, bias=False)
        self.linear1 = nn.Linear(emb_dims, head, bias=False)
        self.bn6 = nn.BatchNorm1d(head)
        self.dp1 = nn.Dropout(p=dropout)
        self.linear2 = nn.Linear(head, out_channel)

    def forward(self, x):
        pool, P = self._ME.pool, self._ME.paconv
        F, boff, idx, rows, csr = self._graph(x)
        h = P.batch_norm_rows(F.mm(self.conv1.weight.view(self.conv1.out_channels, -1).t()), self.bn1, True)
        for i in (2, 3, 4):
            h = self._layer(i, h, rows, idx, csr, "pointnet", 0)
        h = P.batch_norm_rows(h.mm(self.conv5.weight.view(self.conv5.out_channels, -1).t()), self.bn5, True)
        h = pool.GlobalMaxPoolFunction.apply(h, boff)[0]
        h = self.dp1(P.batch_norm_rows(self.linear1(h), self.bn6, True))
        return self.linear2(h)


@gin.configurable
class PAConvDGCNN(_PAConvBase):
    """The reference's `PAConv` of DGCNN_PAConv.py; `in_channel` replaces its hard-coded 3 and `out_channel` its 40."""

    def __init__(self, in_channel, out_channel, k=20, calc_scores="softmax", num_matrices=(8, 8, 8, 8), dropout=0.5,
                 channels=(64, 64, 128, 256), emb_dims=1024, head=(512, 256), ME=None):
        super().__init__(ME)
        ScoreNet = self._ME.paconv.ScoreNet
        assert len(num_matrices) == 4 and len(channels) == 4 and len(head) == 2
        self.k, self.calc_scores = int(k), calc_scores
        self.m1, self.m2, self.m3, self.m4 = num_matrices
        for i, m in enumerate(num_matrices, start=1):
            setattr(self, f"scorenet{i}", ScoreNet(2 * in_channel, m, hidden_unit=[16]))
        cin = in_channel
        for i, (m, c) in enumerate(zip(num_matrices, channels), start=1):
            setattr(self, f"matrice{i}", _bank(m, 2 * cin, c))
            cin = c
        for i, c in enumerate(channels, start=1):
            setattr(self, f"bn{i}", nn.BatchNorm1d(c, momentum=0.1))
        self.bn5 = nn.BatchNorm1d(emb_dims, momentum=0.1)
        self.conv5 = nn.Sequential(nn.Conv1d(sum(channels), emb_dims, kernel_size=1, bias=False), self.bn5)
        self.linear1 = nn.Linear(2 * emb_dims, head[0], bias=False)
        self.bn11 = nn.BatchNorm1d(head[0])
        self.dp1 = nn.Dropout(p=dropout)
        self.linear2 = nn.Linear(head[0], head[1], bias=False)
        self.bn22 = nn.BatchNorm1d(head[1])
        self.dp2 = nn.Dropout(p=dropout)
        self.linear3 = nn.Linear(head[1], out_channel)

    def forward(self, x):
        pool, P = self._ME.pool, self._ME.paconv
        h, boff, idx, rows, csr = self._graph(x)
        outs = []
        for i in (1, 2, 3, 4):
            h = self._layer(i, h, rows, idx, csr, "dgcnn", 0.5)
            outs.append(h)
        conv = self.conv5[0]
        h = P.batch_norm_rows(torch.cat(outs, 1).mm(conv.weight.view(conv.out_channels, -1).t()), self.bn5, True)
        h = torch.cat([pool.GlobalMaxPoolFunction.apply(h, boff)[0], pool.GlobalAvgPoolFunction.apply(h, boff)], 1)
        h = self.dp1(P.batch_norm_rows(self.linear1(h), self.bn11, True))
        h = self.dp2(P.batch_norm_rows(self.linear2(h), self.bn22, True))
        return self.linear3(h)
