"""CRNN recogniser on HIP kernels: the CNN-only recogniser's conv trunk, a 2-layer bidirectional LSTM and a linear layer
(reference: model/cnn_lstm.py:9-103 - the recogniser the reference builds when the `hwr` key is absent).

Output is [T,B,n_class], T = W/4 - 2 (log-probabilities when `use_softmax`). State-dict keys, shapes and the gate layout (i, f, g, o rows of
`weight_ih_l*` / `weight_hh_l*`) are torch.nn.LSTM's, so a reference checkpoint loads with strict=True and one written here loads there. The
LSTM parameters are plain nn.Parameters in nn.LSTM's registration order (nn.LSTM itself re-points parameter storage in
`flatten_parameters`, which would fight the trainer's flat parameter buffer). The recurrence is ops.bilstm: per layer and direction one
ops.linear for the input projection, then one launch per time step of csrc/lstm.hip; between the layers, in train mode, an elementwise
dropout multiplier (p = 0.5) from the Philox stream - torch's own LSTM draws its mask from its own generator, so train-mode outputs are not
comparable sample by sample.
"""
import math

import torch
from torch import nn

from .. import ops
from .cnn_only_hwr import make_trunk, norm_kind_of, run_trunk
from .layers import Linear


class LSTM(nn.Module):
    """parameters of a bidirectional multi-layer torch.nn.LSTM (names, shapes, order and default initialisation), run by ops.bilstm"""

    def __init__(self, input_size, hidden_size, num_layers=2, dropout=0.5):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers, self.dropout = input_size, hidden_size, num_layers, float(dropout)
        for layer in range(num_layers):
            nin = input_size if layer == 0 else 2 * hidden_size
            for suffix in ("", "_reverse"):
                self.register_parameter("weight_ih_l%d%s" % (layer, suffix), nn.Parameter(torch.empty(4 * hidden_size, nin)))
                self.register_parameter("weight_hh_l%d%s" % (layer, suffix), nn.Parameter(torch.empty(4 * hidden_size, hidden_size)))
                self.register_parameter("bias_ih_l%d%s" % (layer, suffix), nn.Parameter(torch.empty(4 * hidden_size)))
                self.register_parameter("bias_hh_l%d%s" % (layer, suffix), nn.Parameter(torch.empty(4 * hidden_size)))
        stdv = 1.0 / math.sqrt(hidden_size)
        for p in self.parameters():
            nn.init.uniform_(p, -stdv, stdv)

    def layer_params(self):
        """per layer ((w_ih, w_hh, b_ih, b_hh) forward, the same four reverse): what ops.bilstm takes"""
        return [tuple(tuple(getattr(self, "%s_l%d%s" % (n, layer, suffix)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                      for suffix in ("", "_reverse")) for layer in range(self.num_layers)]

    def forward(self, x, masks=None):
        """x [T,B,input_size] -> [T,B,2*hidden_size]; masks: the dropout multipliers between the layers when the caller supplies them"""
        return ops.bilstm(x, self.layer_params(), self.dropout, self.training, masks)


class BidirectionalLSTM(nn.Module):
    def __init__(self, nIn, nHidden, nOut):
        super().__init__()
        self.rnn = LSTM(nIn, nHidden, num_layers=2, dropout=0.5)
        self.embedding = Linear(nHidden * 2, nOut)

    def forward(self, input):
        recurrent = self.rnn(input)
        T, b, h = recurrent.shape
        output = self.embedding(recurrent.contiguous().view(T * b, h))
        return output.view(T, b, -1)


class CRNN(nn.Module):
    """for 64-pixel-high lines"""

    def __init__(self, nclass, nc=1, cnnOutSize=512, nh=512, n_rnn=2, leakyRelu=False, norm="batch", use_softmax=False, small=False, pad=False):
        super().__init__()
        if leakyRelu or small:
            raise NotImplementedError("leakyRelu/small recogniser variants are not used by any shipped config")
        self.use_softmax = use_softmax
        if pad == "less":
            self.pad_cols = 64
        elif pad:
            self.pad_cols = 128
        else:
            self.pad_cols = 0
        self.norm_kind = norm_kind_of(norm)
        self.cnn = make_trunk(nc, self.norm_kind)
        self.rnn = BidirectionalLSTM(cnnOutSize, nh, nclass)

    def forward(self, input, style=None):
        with ops.scope("HWR"):
            return self._forward(input, style)

    def _forward(self, input, style=None):
        """input NCHW [B,1,64,W] -> [T,B,n_class], T = W/4 - 2"""
        x = ops.to_nhwc(input)
        if self.pad_cols:
            x = ops.pad2d(x, self.pad_cols, self.pad_cols, 0, 0, "constant", 0.0)
        if x.shape[2] < 12:
            diff = 12 - x.shape[2]
            x = ops.pad2d(x, diff // 2, diff // 2 + diff % 2, 0, 0, "constant", 0.0)
        x = run_trunk(self.cnn, self.norm_kind, x)
        B, H, W, C = x.shape
        if H != 1:
            # the reference flattens (c,h) into channels; only height-1 features are meaningful for the shipped 64-px configs
            raise ValueError("recogniser expects 64-pixel-high lines (feature height %d != 1)" % H)
        out = self.rnn(ops.permute_bl_to_lb(x))                      # [T,B,nclass]
        if not self.use_softmax:
            return out
        T, B, K = out.shape
        # log_softmax_tbc maps NHWC [B',1,T',K] to [T',B',K]: with B' = T*B rows and T' = 1 the row order is kept
        return ops.log_softmax_tbc(out.view(T * B, 1, 1, K)).view(T, B, K)


class SmallCRNN(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()
        raise NotImplementedError("leakyRelu/small recogniser variants are not used by any shipped config")
