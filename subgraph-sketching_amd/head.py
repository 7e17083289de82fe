"""StructureHead: the structure-feature branch of a trained ELPH / BUDDY model, in the form ElphHashes.score_links feeds to the
pair kernel (csrc/ss_head.hpp).

Both reference models do the same with a feature row `sf` the moment they receive it (models/elph.py:73-86 LinkPredictor.forward,
:324-352 BUDDY.forward):

    x = relu(bn_labels(label_lin_layer(sf)))            # dim -> dim
    logit = lin(cat([x, feature branch, embedding branch, RA]))

`lin` is linear over the concatenation and the label branch comes first, so its share of the logit is lin.weight[0, :dim] . x -- one
float per link that depends on the sketches and ~1 000 floats of weights only.  In eval mode BatchNorm is an affine map, folded
here into the linear layer on the host in float64:

    s = bn_weight / sqrt(bn_var + eps);   W' = s[:, None] * weight;   t' = (bias - bn_mean) * s + bn_bias
    score = b2 + sum_j w2[j] * max(0, t'[j] + sum_i W'[j][i] * x[i])

Inference only: batch statistics (training mode) cannot be folded and the kernel has no gradients.
"""
import ctypes

import numpy as np
import torch

from . import _native


def _vec64(t, name, n=None):
    a = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)
    if a.ndim != 1 or (n is not None and a.shape[0] != n):
        raise ValueError(f'{name} must have shape [{n if n is not None else "dim"}], got {tuple(a.shape)}')
    return a


class _DeviceHead(object):
    """the folded parameters resident on one device (struct ss_structure_head + the tensors it points to)"""

    def __init__(self, head, device):
        self.w1 = torch.from_numpy(head.w1).to(device)
        self.shift = torch.from_numpy(head.shift).to(device)
        self.w2 = torch.from_numpy(head.w2).to(device)
        self.struct = _native.StructureHeadStruct(dim=head.dim, normalised=int(head.normalised), w1=self.w1.data_ptr(),
                                                  shift=self.shift.data_ptr(), w2=self.w2.data_ptr(), bias=head.b2)


class StructureHead(object):
    """One trained structure branch: label_lin_layer (weight [dim, dim], bias [dim]), bn_labels in eval mode (bn_weight, bn_bias,
    bn_mean, bn_var [dim], bn_eps) and the label branch's columns of the output layer (out_weight [dim] = lin.weight[0, :dim];
    out_bias = lin.bias, or None when the caller adds the bias with the other branches).  dim = h(h+2) for an h in {1, 2, 3}, or
    2 h(h+2) with normalised=True (BUDDY's add_normed_features: the row carries its degree-normalised copy).

    Attributes (numpy float32, host): w1 [dim, dim] = W', shift [dim] = t', w2 [dim]; b2 (float); dim, hops, normalised."""

    def __init__(self, weight, bias, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, out_weight, out_bias=None, normalised=False):
        w = (weight.detach().cpu().numpy() if isinstance(weight, torch.Tensor) else np.asarray(weight)).astype(np.float64)
        if w.ndim != 2 or w.shape[0] != w.shape[1]:
            raise ValueError(f'weight must be square [dim, dim], got {tuple(w.shape)}')
        dim = int(w.shape[0])
        self.normalised = bool(normalised)
        widths = {(2 if self.normalised else 1) * h * (h + 2): h for h in (1, 2, 3)}
        if dim not in widths:
            raise ValueError(f'dim = {dim} is not {"2 " if self.normalised else ""}h(h+2) for an h in {{1, 2, 3}} '
                             f'(normalised={self.normalised}): expected one of {sorted(widths)}')
        self.dim, self.hops = dim, widths[dim]
        b, g, beta, mean, var = (_vec64(t, n, dim) for t, n in ((bias, 'bias'), (bn_weight, 'bn_weight'), (bn_bias, 'bn_bias'),
                                                                 (bn_mean, 'bn_mean'), (bn_var, 'bn_var')))
        ow = (out_weight.detach().cpu().numpy() if isinstance(out_weight, torch.Tensor) else np.asarray(out_weight)).astype(np.float64)
        ow = ow.reshape(-1) if ow.ndim == 2 and ow.shape[0] == 1 else ow
        if ow.ndim != 1 or ow.shape[0] != dim:
            raise ValueError(f'out_weight must have shape [{dim}] (the first dim columns of lin.weight[0]), got {tuple(ow.shape)}')
        s = g / np.sqrt(var + float(bn_eps))
        self.w1 = np.ascontiguousarray((s[:, None] * w).astype(np.float32))
        self.shift = ((b - mean) * s + beta).astype(np.float32)
        self.w2 = ow.astype(np.float32)
        if out_bias is None:
            self.b2 = 0.0
        else:
            ob = (out_bias.detach().cpu().numpy() if isinstance(out_bias, torch.Tensor) else np.asarray(out_bias)).astype(np.float64)
            if ob.size != 1:
                raise ValueError(f'out_bias must be one number, got shape {tuple(ob.shape)}')
            self.b2 = float(np.float32(ob.reshape(-1)[0]))
        self._dev = {}

    @classmethod
    def from_module(cls, m):
        """the head of a model with the reference's attribute names (both LinkPredictor and BUDDY have them): m.label_lin_layer,
        m.bn_labels, m.lin, m.dim, and m.append_normalised where it exists.  Duck-typed: nothing of the reference is imported."""
        if getattr(m, 'training', False):
            raise ValueError('the model is in training mode: BatchNorm batch statistics cannot be folded (call model.eval())')
        dim = int(m.dim)
        lin1, bn, lin = m.label_lin_layer, m.bn_labels, m.lin
        if tuple(lin1.weight.shape) != (dim, dim):
            raise ValueError(f'label_lin_layer.weight must be [{dim}, {dim}] (m.dim = {dim}), got {tuple(lin1.weight.shape)}')
        if int(lin.in_features) < dim:
            raise ValueError(f'lin has {int(lin.in_features)} input features, fewer than the label branch (m.dim = {dim})')
        if lin.weight.dim() != 2 or lin.weight.shape[0] != 1 or lin.weight.shape[1] < dim:
            raise ValueError(f'lin.weight must be [1, >= {dim}], got {tuple(lin.weight.shape)}')
        if bn.running_mean is None or bn.running_var is None:
            raise ValueError('bn_labels keeps no running statistics: nothing to fold')
        ones, zeros = torch.ones(dim, dtype=torch.float64), torch.zeros(dim, dtype=torch.float64)
        return cls(lin1.weight, lin1.bias if lin1.bias is not None else zeros,
                   bn.weight if bn.weight is not None else ones, bn.bias if bn.bias is not None else zeros,
                   bn.running_mean, bn.running_var, bn.eps, lin.weight[0, :dim], out_bias=lin.bias,
                   normalised=bool(getattr(m, 'append_normalised', False)))

    def _device(self, device):
        """the device copy, one per device (as the engine caches its estimator tables)"""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = _DeviceHead(self, device)
        return self._dev[key]

    def reference(self, x):
        """float64 numpy evaluation of the folded head on rows x [L, dim] (tests, spot checks; not a compute path)"""
        x = np.asarray(x, dtype=np.float64)
        hidden = np.maximum(x @ self.w1.astype(np.float64).T + self.shift.astype(np.float64), 0.0)
        return hidden @ self.w2.astype(np.float64) + self.b2

    # no device handles in pickled state
    def __getstate__(self):
        state = dict(self.__dict__)
        state['_dev'] = {}
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._dev = {}


assert ctypes.sizeof(_native.StructureHeadStruct) == 40  # {int32, int32, 3 pointers, float, padding}: struct ss_structure_head
