"""GRU4Rec, DIN, DIEN, SLi-Rec, A2SVD, Caser, NCF and NextItNet on the kernels of the CLSR step.

The reference's quick-start trains these from the same script as CLSR (examples/00_quick_start/sequential.py:94-205);
they sit on the same ``SequentialBaseModel`` trunk (embeddings + involved-row regulariser + logit MLP + softmax loss +
clip + Adam) and differ in ``_build_seq_graph``:

  GRU4RecModel   models/sequential/gru4rec.py:21-76     dynamic_rnn(GRUCell) final state ++ target
  DINModel       models/sequential/din.py:13-34          target ++ masked history sum ++ _attention_fcn(target, history)
  A2SVDModel     models/sequential/asvd.py:13-45         A2SVD attention ++ target
  DIENModel      models/sequential/dien.py:13-64         GRU -> _attention_fcn WEIGHTS -> attentional GRU (one sequence
                                                         per candidate row) final state, ++ target, history sum, product
  SLI_RECModel   models/sequential/sli_rec.py:25-147     A2SVD attention (unmasked), Time4LSTM over the item embedding,
                                                         _attention_fcn(target, rnn_outputs), alpha fusion
  CaserModel     models/sequential/caser.py:37-106       per table: one dense contraction of the flattened history
                                                         ("vertical") ++ width-1..L convolutions, ReLU, max over time
                                                         ("horizonal"), ++ target -- no mask anywhere
  NCFModel       models/sequential/ncf.py:15-103         four id tables of its own: user_gmf * item_gmf ++ a ReLU tower
                                                         over user_mlp ++ item_mlp; one bias-free output layer, no
                                                         history encoder, no logit MLP, no batch-norm
  NextItNetModel models/sequential/nextitnet.py:21-232   a stack of residual blocks (layer norm, ReLU, 1x1 conv, causal dilated
                                                         conv, 1x1 conv) over the history; trained on EVERY position: the
                                                         logit MLP sees Hn T G rows -- no mask anywhere

  SASRecModel    (no reference file: the paper's baseline)  a learnt position row, then blocks of causal self-attention and a
                                                         ReLU feed-forward (pre-norm, residual), a final layer norm on the
                                                         last valid step, ++ target; padding masked everywhere
                                                         (csrc/sasrec.hip); ``long_histories=True``:
                                                         histories past what LDS holds run the tiled kernels, up to 256

``SeqNet`` re-uses CLSRNet wholesale -- parameter store, packed weights, the position-tiled GEMMs, the fused recurrence
launch, the attention block (forward and backward), the MLP heads, sorted segmented embedding gradients, regularisers,
clip, Adam, the stream structure, data parallelism -- and only re-states the three graphs and their backward passes.
New device code: the A2SVD attention and the length scaling of DIN's history sum (csrc/sibling.hip); Caser's
convolutions, forward and backward (csrc/caser.hip); all of NCF between the ids and the per-line
gradient slices (csrc/ncf.hip, DESIGN.md section 9c: one launch to score, two to train); NextItNet's whole stack of blocks,
one launch forward and one backward (csrc/nextitnet.hip).

A2SVD and GRU4Rec, whose one ``_fcn_net`` is the logit MLP, also train with the config's dropout (``user_dropout``,
``dropout``: csrc/dropout.hip, ``CLSRNet._mlp_fwd_drop``); the others refuse it by name
(Caser for now: its tail is the same one).

  LGNModel       models/sequential/lgn.py:47-132         kind "lgn": no history encoder and no logit MLP either.  All Vu + Vi
                                                         rows [user_embedding ; item ++ cate[item2cate]] go twice through the
                                                         normalised user-item adjacency (``graph=``, clsr_amd/lgn_graph.py) and
                                                         a C x C layer; logit = F[user] . F[Vu + item] (csrc/lgn.hip)
"""
import copy

import numpy as np
import torch

from clsr_amd import ops
from clsr_amd.net import CLSRNet, _StepState, _pad4
from clsr_amd.ops import call, query
from clsr_amd.params import UNUSED_TABLE, nextitnet_block_scope, sibling_kind, sibling_scopes, sibling_specs, sibling_tables

LG = "sequential/logit_fcn/nn_part/"


class SeqNet(CLSRNet):
    def __init__(self, hp, dims, kind=None, **kw):
        self.kind = sibling_kind(kind if kind is not None else hp.model_type)
        if self.kind is None:
            raise ValueError("SeqNet builds gru4rec / din / dien / sli_rec / a2svd / caser / ncf / nextitnet / lgn / sasrec, got %r"
                             % (kind or hp.model_type,))
        self.sc = sibling_scopes(self.kind)
        if self.kind == "caser" and hp.hidden_size is None:
            hp = copy.copy(hp)
            hp.hidden_size = 0         # (caser.yaml has no recurrent encoder: nothing reads the width)
        if self.kind == "ncf":
            # settings without effect in NCF's graph (ncf.py never reads them): whatever they hold, the trunk sees values
            # it can unpack and no dropout
            hp = copy.copy(hp)
            hp.hidden_size, hp.user_dropout, hp.embedding_dropout = hp.hidden_size or 0, False, 0.0
            if len(hp.layer_sizes or ()) != 2:
                hp.layer_sizes = [4, 4]
            if len(hp.att_fcn_layer_sizes or ()) != 2:
                hp.att_fcn_layer_sizes = None
        self._lg_graph = kw.pop("graph", None)
        # SASRec only: histories past what LDS holds run the tiled kernels (csrc/sasrec.hip)
        self.long_histories = bool(kw.pop("long_histories", False))
        if self.long_histories and self.kind != "sasrec":
            raise NotImplementedError("long_histories=True is SASRec's keyword (kind 'sasrec'): %s takes its histories of up "
                                      "to 256 steps as it is" % self.kind)
        if self.kind == "lgn":
            # settings without effect in LGN's graph (lgn.py never reads them): whatever they hold, the trunk sees values it
            # can unpack and no dropout in an MLP that does not exist (embedding_dropout stays as it is: refused when set)
            hp = copy.copy(hp)
            hp.hidden_size, hp.user_dropout = hp.hidden_size or 0, False
            if len(hp.layer_sizes or ()) != 2:
                hp.layer_sizes = [4, 4]
            if len(hp.att_fcn_layer_sizes or ()) != 2:
                hp.att_fcn_layer_sizes = None
        if self.kind == "nextitnet":
            # settings without effect in NextItNet's graph (nextitnet.py never reads them): whatever they hold, the trunk
            # sees values it can unpack
            hp = copy.copy(hp)
            hp.hidden_size, hp.att_fcn_layer_sizes = 0, None       # (attention_size: the trunk never reads it for this kind)
        if self.kind == "sasrec":
            # settings the encoder never reads: whatever they hold, the trunk sees values it can unpack
            hp = copy.copy(hp)
            hp.hidden_size, hp.att_fcn_layer_sizes = 0, None       # (attention_size: the trunk never reads it for this kind)
        super(SeqNet, self).__init__(hp, dims, **kw)
        if self.kind == "sasrec":
            self._sasrec_setup()
        if self.kind == "caser":
            self._caser_setup()
        if self.kind == "nextitnet":
            self._nextitnet_setup()
        if self.kind == "ncf":
            self._ncf_setup()
        if self.kind == "lgn":
            self._lgn_setup()
        if self.kind == "sli_rec":
            self.enc_in = self.Di          # Time4LSTM reads the item embedding only (sli_rec.py:43-57)
        self.split_query = False

    # ------------------------------------------------------------------ configuration
    def _check_supported(self):
        hp, bad = self.hp, []
        if self.kind == "ncf":
            bad = self._ncf_limits(hp)
            if bad:
                raise NotImplementedError("ncf HIP path does not support: " + "; ".join(bad))
            return
        if self.kind == "lgn":
            bad = self._lgn_limits(hp)
            if bad:
                raise NotImplementedError("lgn HIP path does not support: " + "; ".join(bad))
            return
        if hp.enable_BN is not True:
            bad.append("enable_BN must be True")
        if list(hp.activation) != ["relu"] * len(hp.activation):
            bad.append("activation must be relu")
        self._check_dropout(hp, bad, mlp_only=self.kind in ("a2svd", "gru4rec", "caser", "nextitnet", "sasrec"))
        if self.kind in ("caser", "nextitnet", "sasrec") and self.dropout_in_effect(hp):
            # (its one _fcn_net is the logit MLP too: the tail of A2SVD / GRU4Rec would serve; not wired up or tested yet)
            bad.append("user_dropout with dropout %r: dropout in %s's logit MLP is not implemented yet"
                       % ([float(d) for d in hp.dropout],
                          {"caser": "Caser", "nextitnet": "NextItNet", "sasrec": "SASRec"}[self.kind]))
        if self.kind == "nextitnet" and self.precision != "fp32":
            bad.append("precision must be 'fp32', got %r (NextItNet's kernels are fp32 FMA chains)" % (self.precision,))
        if self.kind == "sasrec" and self.precision != "fp32":
            bad.append("precision must be 'fp32', got %r (SASRec's kernels are fp32 FMA chains)" % (self.precision,))
        if any(float(getattr(hp, k)) != 0.0 for k in ("embed_l1", "layer_l1", "cross_l1", "cross_l2")):
            bad.append("l1 / cross regularisers must be 0")
        if hp.loss != "softmax" or hp.method != "classification":
            bad.append("loss must be softmax / method classification")
        if len(hp.layer_sizes) != 2:
            bad.append("layer_sizes must have two layers")
        D = hp.item_embedding_dim + hp.cate_embedding_dim
        if self.kind in ("din", "sli_rec", "dien") and len(hp.att_fcn_layer_sizes or ()) != 2:
            bad.append("att_fcn_layer_sizes must have two layers")
        if self.kind == "a2svd" and hp.attention_size != D:
            bad.append("attention_size must equal item+cate dims (tensordot with query, base_model.py:622)")
        if self.kind == "sli_rec":
            if hp.hidden_size != D:
                bad.append("hidden_size must equal item+cate dims (alpha fusion of att_fea1 and att_fea2, sli_rec.py:92)")
            if hp.attention_size != D:
                bad.append("attention_size must equal item+cate dims (tensordot with query, base_model.py:622)")
        bad += self._shape_limits(hp, rnn=self.kind in ("gru4rec", "sli_rec", "dien"))
        if self.kind == "caser":
            bad += self._caser_limits(hp, bool(bad))
        if self.kind == "nextitnet":
            bad += self._nextitnet_limits(hp)
        if self.kind == "sasrec":
            bad += self._sasrec_limits(hp, self.long_histories)
        if self.kind in ("a2svd", "sli_rec") and int(hp.attention_size) % 4:
            bad.append("attention_size must be a multiple of 4")
        if bad:
            raise NotImplementedError("%s HIP path does not support: %s" % (self.kind, "; ".join(bad)))

    @staticmethod
    def _caser_limits(hp, trunk_bad):
        """Caser's own keys, by name; the kernels' say on the whole shape (csrc/caser.hip) once each key is in range."""
        bad = []
        if any(getattr(hp, k, None) is None for k in ("L", "n_v", "n_h")):
            return ["L, n_v and n_h must be set (caser.yaml: L 3, n_v 128, n_h 128)"]
        L, n_v, n_h, T = int(hp.L), int(hp.n_v), int(hp.n_h), int(hp.max_seq_length)
        fmax = query("clsr_caser_max_filters")
        if not 1 <= L <= T:
            bad.append("L must lie in 1..max_seq_length (%d), got %d" % (T, L))
        for k, v in (("n_v", n_v), ("n_h", n_h)):
            if v <= 0 or v % 4 or v > fmax:
                bad.append("%s must be a positive multiple of 4, at most %d, got %d" % (k, fmax, v))
        if not bad and not trunk_bad and not query("clsr_caser_supported", T, int(hp.item_embedding_dim),
                                                   int(hp.cate_embedding_dim), L, n_v, n_h):
            bad.append("L = %d with embedding dims %d / %d and n_v, n_h = %d, %d: a chunk of 8 positions plus L - 1 rows of "
                       "the wider table must fit 64 KB of LDS, and n_v + 3 L n_h must be at most 16 384"
                       % (L, int(hp.item_embedding_dim), int(hp.cate_embedding_dim), n_v, n_h))
        return bad

    @staticmethod
    def _nextitnet_limits(hp):
        """NextItNet's own keys, by name; the kernels' say on the whole shape (csrc/nextitnet.hip) once each key is in
        range.  hidden_size, attention_size and att_fcn_layer_sizes are never read: any value passes."""
        bad = []
        if not getattr(hp, "dilations", None) or getattr(hp, "kernel_size", None) is None:
            return ["dilations and kernel_size must be set (nextitnet.yaml: dilations [1, 2, 4, 1, 2, 4], kernel_size 3)"]
        cmax, kmax, nbmax = (query("clsr_nextitnet_max_" + n) for n in ("channels", "kernel", "blocks"))
        dil, k = list(hp.dilations), hp.kernel_size
        ok_d = all(isinstance(d, (int, np.integer)) and not isinstance(d, bool) and d >= 1 for d in dil)
        if not 1 <= len(dil) <= nbmax or not ok_d:
            bad.append("dilations must hold 1 to %d positive integers, got %r" % (nbmax, dil))
        if not isinstance(k, (int, np.integer)) or not 1 <= k <= kmax:
            bad.append("kernel_size must lie in 1..%d, got %r" % (kmax, k))
        Di, Dc, T = int(hp.item_embedding_dim), int(hp.cate_embedding_dim), int(hp.max_seq_length)
        C = Di + Dc
        if Di <= 0 or Dc <= 0 or C % 8 or C > cmax:
            bad.append("item_embedding_dim + cate_embedding_dim must be a multiple of 8, at most %d (half of it is the "
                       "blocks' inner width), got %d + %d" % (cmax, Di, Dc))
        ngs = int(hp.train_num_ngs)
        if not 1 <= ngs <= 255:
            bad.append("train_num_ngs must lie in 1..255 (every position is a softmax group of 1 + train_num_ngs rows), "
                       "got %d" % ngs)
        if not bad and 1 <= T <= 256 and not query("clsr_nextitnet_supported", T, C, int(k), len(dil),
                                                              min(int(max(dil)), 1 << 20)):
            bad.append("max_seq_length %d with item_embedding_dim + cate_embedding_dim = %d: a history's backward state needs "
                       "%d bytes of LDS, the budget is %d (64 KB)"
                       % (T, C, query("clsr_nextitnet_lds_bytes", T, C, 1), query("clsr_nextitnet_lds_budget_bytes")))
        return bad

    def _nextitnet_setup(self):
        """NextItNet's shape constants and the parameter block the kernels address by offset: the variables of all blocks
        are consecutive in the dense buffer, in the layout csrc/nextitnet.hip states (checked here, once)."""
        hp = self.hp
        self.nx_T, self.nx_k, self.nx_nb = int(hp.max_seq_length), int(hp.kernel_size), len(hp.dilations)
        names = [n for n, _, _ in self.specs if n.startswith(self.sc["nx"])]
        first, o = self.P[names[0]], 0
        for n in names:
            if self.P[n].data_ptr() != first.data_ptr() + 4 * o:
                raise AssertionError("NextItNet parameter block is not contiguous at %s" % n)
            o += self.P[n].numel()
        if o != query("clsr_nextitnet_param_floats", self.D, self.nx_k, self.nx_nb):
            raise AssertionError("NextItNet parameter block: %d floats" % o)
        if first.data_ptr() % 16:
            raise AssertionError("NextItNet parameter block is not 16-byte aligned")
        if not names[0].startswith(nextitnet_block_scope(self.sc["nx"], 0, int(hp.dilations[0])) + "layer_norm1/beta"):
            raise AssertionError("NextItNet parameter block starts at %s" % names[0])
        g0 = (self.Gd[names[0]].data_ptr() - self.dense_grad.data_ptr()) // 4
        self.nx_W, self.nx_dW, self.nx_P = first, self.dense_grad[g0:g0 + o], o
        # (a rate of T or more only ever reads the padding: every such rate computes what T does)
        self.nx_dil = torch.tensor([min(int(d), 1 << 20) for d in hp.dilations], dtype=torch.int32, device=self.device)

    @staticmethod
    def _sasrec_limits(hp, long_histories=False):
        """SASRec's own keys, by name; the kernels' say on the whole shape (csrc/sasrec.hip) once each key is in range.
        hidden_size, attention_size, att_fcn_layer_sizes and attention_dropout are never read: any value passes.
        ``long_histories``: a shape the resident kernels refuse passes if the tiled ones hold it under their default tile."""
        bad = []
        nb, nh = getattr(hp, "num_blocks", None), getattr(hp, "num_heads", None)
        if nb is None or nh is None:
            return ["num_blocks and num_heads must be set (sasrec.yaml: num_blocks 2, num_heads 1)"]
        cmax, nbmax, tmax = (query("clsr_sasrec_max_" + n) for n in ("channels", "blocks", "steps"))
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if not is_int(nb) or not 1 <= nb <= nbmax:
            bad.append("num_blocks must lie in 1..%d, got %r" % (nbmax, nb))
        Di, Dc, T = int(hp.item_embedding_dim), int(hp.cate_embedding_dim), int(hp.max_seq_length)
        C = Di + Dc
        if Di <= 0 or Dc <= 0 or C % 8 or C > cmax:
            bad.append("item_embedding_dim + cate_embedding_dim must be a multiple of 8, at most %d, got %d + %d"
                       % (cmax, Di, Dc))
        elif not is_int(nh) or nh < 1 or C % nh or (C // nh) % 4:
            bad.append("num_heads must divide item_embedding_dim + cate_embedding_dim = %d into heads of a multiple of 4 "
                       "channels, got %r" % (C, nh))
        if not bad and 1 <= T <= tmax and not query("clsr_sasrec_supported", T, T, C, int(nb), int(nh)):
            if not long_histories:
                bad.append("max_seq_length %d with item_embedding_dim + cate_embedding_dim = %d: a history's backward state "
                           "needs %d bytes of LDS, the budget is %d (160 KB); long_histories=True lifts this limit (tiled "
                           "kernels, up to %d steps)"
                           % (T, C, query("clsr_sasrec_lds_bytes", T, C, 1), query("clsr_sasrec_lds_budget_bytes"), tmax))
            elif query("clsr_sasrec_tiled_default_tile", T, C) <= 0:
                bad.append("max_seq_length %d with item_embedding_dim + cate_embedding_dim = %d: k and v of a history and one "
                           "row of the tiled backward's state need %d bytes of LDS, the budget is %d (160 KB)"
                           % (T, C, query("clsr_sasrec_tiled_lds_bytes", T, C, 1, 1), query("clsr_sasrec_lds_budget_bytes")))
        return bad

    def _sasrec_setup(self):
        """SASRec's shape constants and the parameter block the kernels address by offset: the positional table, the
        variables of all blocks and the final layer norm are consecutive in the dense buffer, in the layout csrc/sasrec.hip
        states (checked here, once)."""
        hp = self.hp
        self.sa_T, self.sa_nb, self.sa_nh = int(hp.max_seq_length), int(hp.num_blocks), int(hp.num_heads)
        names = [n for n, _, _ in self.specs if n.startswith(self.sc["sa"])]
        first, o = self.P[names[0]], 0
        for n in names:
            if self.P[n].data_ptr() != first.data_ptr() + 4 * o:
                raise AssertionError("SASRec parameter block is not contiguous at %s" % n)
            o += self.P[n].numel()
        if o != query("clsr_sasrec_param_floats", self.sa_T, self.D, self.sa_nb):
            raise AssertionError("SASRec parameter block: %d floats" % o)
        if first.data_ptr() % 16:
            raise AssertionError("SASRec parameter block is not 16-byte aligned")
        if names[0] != self.sc["sa"] + "position_embedding" or names[-1] != self.sc["sa"] + "layer_norm_final/bias":
            raise AssertionError("SASRec parameter block runs from %s to %s" % (names[0], names[-1]))
        g0 = (self.Gd[names[0]].data_ptr() - self.dense_grad.data_ptr()) // 4
        self.sa_W, self.sa_dW, self.sa_P = first, self.dense_grad[g0:g0 + o], o

    def _sasrec_tile(self, T):
        """The pair of kernels a feed of T steps runs, forward and backward alike: 0, the resident pair, for every shape it
        admits (a net built with ``long_histories`` is bit-identical to one without there), else the tiled pair's tile."""
        if not self.long_histories or query("clsr_sasrec_supported", T, self.sa_T, self.D, self.sa_nb, self.sa_nh):
            return 0
        return query("clsr_sasrec_tiled_default_tile", T, self.D)

    @staticmethod
    def _ncf_widths(hp):
        """(Du, number of tower layers, the four width arguments of the clsr_ncf_* entry points)"""
        sizes = [int(w) for w in (hp.ncf_layer_sizes or ())]
        return int(hp.user_embedding_dim), len(sizes), tuple((sizes + [0, 0, 0, 0])[:4])

    @classmethod
    def _ncf_limits(cls, hp):
        """What NCF's graph reads, by key name; the kernel's say on the whole shape (csrc/ncf.hip) once each key is in range.
        layer_sizes, activation, enable_BN, the dropout keys, att_fcn_layer_sizes, hidden_size and attention_size are never
        read by the reference's NCF: any value passes."""
        bad = []
        if any(float(getattr(hp, k)) != 0.0 for k in ("embed_l1", "layer_l1", "cross_l1", "cross_l2")):
            bad.append("l1 / cross regularisers must be 0")
        if hp.loss != "softmax" or hp.method != "classification":
            bad.append("loss must be softmax / method classification")
        Di, Dc = int(hp.item_embedding_dim), int(hp.cate_embedding_dim)
        if Di % 4 or Dc % 4 or Di <= 0 or Dc <= 0 or Di + Dc > 256:
            bad.append("item / cate embedding dims must be positive multiples of 4, at most 256 together")
        if int(hp.max_seq_length) > 256:
            bad.append("max_seq_length must be at most 256")
        wmax, lmax, gmax = query("clsr_ncf_max_width"), query("clsr_ncf_max_layers"), query("clsr_ncf_max_group")
        Du, nl, w4 = cls._ncf_widths(hp)
        sizes = [int(w) for w in (hp.ncf_layer_sizes or ())]
        if Du <= 0 or Du % 4 or Du > wmax:
            bad.append("user_embedding_dim must be a positive multiple of 4, at most %d, got %d" % (wmax, Du))
        if not 1 <= nl <= lmax:
            bad.append("ncf_layer_sizes must hold 1 to %d layers, got %d" % (lmax, nl))
        if any(w <= 0 or w % 4 or w > wmax for w in sizes):
            bad.append("ncf_layer_sizes must be positive multiples of 4, at most %d, got %r" % (wmax, sizes))
        G = int(hp.train_num_ngs) + 1
        if not 1 <= G <= gmax:
            bad.append("train_num_ngs must be at most %d (a softmax group of %d lines is one tile of the kernel), got %d"
                       % (gmax - 1, gmax, G - 1))
        if not bad and not query("clsr_ncf_supported", Du, nl, *w4, G):
            bad.append("user_embedding_dim %d with ncf_layer_sizes %r: the tower's weights and a tile of 16 lines need %d "
                       "words of LDS, the budget is %d (64 KB)"
                       % (Du, sizes, query("clsr_ncf_lds_floats", Du, nl, *w4), query("clsr_ncf_lds_budget_floats")))
        return bad

    def _lgn_limits(self, hp):
        """What LGN's graph reads, by key name.  layer_sizes, activation, enable_BN, user_dropout / dropout, hidden_size,
        attention_size and the other models' keys are never read by the reference's LGN: any value passes."""
        from clsr_amd.net import resolve_optimizer

        bad = []
        if any(float(getattr(hp, k)) != 0.0 for k in ("embed_l1", "layer_l1", "cross_l1", "cross_l2")):
            bad.append("l1 / cross regularisers must be 0")
        if hp.loss != "softmax" or hp.method != "classification":
            bad.append("loss must be softmax / method classification")
        if float(hp.embedding_dropout or 0.0) != 0.0:
            bad.append("embedding_dropout must be 0 (no model of this project has embedding dropout), got %r" % (hp.embedding_dropout,))
        Di, Dc, Du = int(hp.item_embedding_dim), int(hp.cate_embedding_dim), int(hp.user_embedding_dim)
        cmax = query("clsr_lgn_max_width")
        if Di <= 0 or Dc <= 0 or Di % 4 or Dc % 4 or Di + Dc > cmax:
            bad.append("item_embedding_dim and cate_embedding_dim must be positive multiples of 4, at most %d together, got %d + %d"
                       % (cmax, Di, Dc))
        if Du != Di + Dc:
            bad.append("user_embedding_dim must equal item_embedding_dim + cate_embedding_dim (the tables are concatenated "
                       "along rows into one node table), got %d against %d + %d" % (Du, Di, Dc))
        if self.precision != "fp32":
            bad.append("precision must be 'fp32', got %r (LGN's kernels are fp32 FMA chains)" % (self.precision,))
        if resolve_optimizer(hp.optimizer) not in ("adam", "lazyadam"):
            bad.append("optimizer must be adam or lazyadam, got %r" % (hp.optimizer,))
        if int(hp.max_seq_length) > 256:
            bad.append("max_seq_length must be at most 256")
        return bad

    def _lgn_setup(self):
        """The device image of the graph (clsr_amd/lgn.py: Propagation), item2cate and its sorted form for the category
        gradient's segment sums, the id lists that mark every row of the two dense-gradient tables, and the parameter
        block: W_gc_k | b_gc_k consecutive in the dense gradient buffer, the layout of a partial row of csrc/lgn.hip."""
        from clsr_amd import lgn

        g, dev = self._lg_graph, self.device
        if g is None:
            raise ValueError("SeqNet kind 'lgn' needs the user-item graph: SeqNet(..., graph=lgn_graph.build_graph(hparams))")
        Vu, Vi, Vc, C = self.dims["Vu"], self.dims["Vi"], self.dims["Vc"], self.D
        i2c = np.ascontiguousarray(g.item2cate, dtype=np.int32)
        if len(g.indptr) - 1 != Vu + Vi or i2c.shape != (Vi,) or (len(i2c) and (i2c.min() < 0 or i2c.max() >= Vc)):
            raise ValueError("graph: expected %d + %d rows and item2cate [%d] with values below %d" % (Vu, Vi, Vi, Vc))
        self.lg_prop = lgn.Propagation(g, C, device=dev)        # (refuses rows / entries past int32 by name)
        i32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=dev)
        self.lg_i2c, self.lg_all_users, self.lg_all_items = i32(i2c), i32(np.arange(Vu)), i32(np.arange(Vi))
        # item2cate never changes: sorted once; category c owns the items perm[seg[c] .. seg[c + 1])
        seg = np.zeros(Vc + 1, dtype=np.int64)
        np.cumsum(np.bincount(i2c, minlength=Vc), out=seg[1:])
        self.lg_cate = lgn._Csr(seg, np.argsort(i2c, kind="stable"), None, self.Dc, dev)
        # involved items | involved categories, one buffer (zeroed together): the rows the regulariser reaches -- of F's
        # item part and of the raw cate_embedding; the table flags say which rows an update visits, which is more
        self.lg_inv_all = torch.zeros(_pad4(Vi) + _pad4(Vc), dtype=torch.uint8, device=dev)
        self.lg_inv, self.lg_inv_c = self.lg_inv_all[:_pad4(Vi)], self.lg_inv_all[_pad4(Vi):]
        self.lg_stats = torch.zeros(query("clsr_lgn_stats_workspace_doubles"), dtype=torch.float64, device=dev)
        sc, pf = self.sc["gc"], self.lg_prop.part_floats
        self.lg_W = [self.P[sc + "W_gc_%d" % k] for k in range(lgn.N_LAYERS)]
        self.lg_b = [self.P[sc + "b_gc_%d" % k] for k in range(lgn.N_LAYERS)]
        self.lg_dWb = []
        for k in range(lgn.N_LAYERS):
            gw, gb = self.Gd[sc + "W_gc_%d" % k], self.Gd[sc + "b_gc_%d" % k]
            if gb.data_ptr() != gw.data_ptr() + 4 * C * C:
                raise AssertionError("LGN parameter block of layer %d is not contiguous" % k)
            g0 = (gw.data_ptr() - self.dense_grad.data_ptr()) // 4
            self.lg_dWb.append(self.dense_grad[g0:g0 + pf])
        self.lg_F, self.lg_F_valid = None, False

    def _ncf_setup(self):
        """NCF's shape constants and the parameter block the kernel addresses by offset: tower weights and biases, then the
        output weights, consecutive in the dense buffer in the layout csrc/ncf.hip states (checked here, once)."""
        self.nc_Du, self.nc_nl, self.nc_w4 = self._ncf_widths(self.hp)
        names = [n for n, _, _ in self.specs if n.startswith(self.sc["fc"])]
        first, o = self.P[names[0]], 0
        for n in names:
            if self.P[n].data_ptr() != first.data_ptr() + 4 * o:
                raise AssertionError("NCF parameter block is not contiguous at %s" % n)
            o += self.P[n].numel()
        if o != query("clsr_ncf_param_floats", self.nc_Du, self.nc_nl, *self.nc_w4):
            raise AssertionError("NCF parameter block: %d floats" % o)
        g0 = (self.Gd[names[0]].data_ptr() - self.dense_grad.data_ptr()) // 4
        self.nc_W, self.nc_dW, self.nc_P = first, self.dense_grad[g0:g0 + o], o

    def _caser_setup(self):
        """Caser's shape constants and the two parameter blocks the kernels address by offset: the variables of a table are
        consecutive in the dense buffer, in the layout csrc/caser.hip states (checked here, once)."""
        hp = self.hp
        self.cz_L, self.cz_nv, self.cz_nh = int(hp.L), int(hp.n_v), int(hp.n_h)
        self.cz_T = int(hp.max_seq_length)
        self.cz_pw = self.cz_nv + self.cz_L * self.cz_nh          # pooled columns of one table
        self.cz_W, self.cz_dW = {}, {}
        for key, Dx in (("item", self.Di), ("cate", self.Dc)):
            names = [n for n, _, _ in self.specs if n.startswith(self.sc[key])]
            first, o = self.P[names[0]], 0
            for n in names:
                if self.P[n].data_ptr() != first.data_ptr() + 4 * o:
                    raise AssertionError("Caser parameter block of %s is not contiguous at %s" % (key, n))
                o += self.P[n].numel()
            if o != query("clsr_caser_param_floats", self.cz_T, Dx, self.cz_L, self.cz_nv, self.cz_nh):
                raise AssertionError("Caser parameter block of %s: %d floats" % (key, o))
            self.cz_W[key], self.cz_dW[key] = first, self.Gd[names[0]]

    def _param_specs(self):
        return sibling_specs(self.dims, self.hp, self.kind)

    def _table_map(self):
        return sibling_tables(self.kind)

    def _unused_tables(self):
        return () if self.kind == "lgn" else (UNUSED_TABLE,)      # (LGN trains user_embedding)

    def _update_spec(self):
        trunk = (("item", None, 4, 0.0, 0.0, None, 0, 3), ("cate", None, 5, 0.0, 0.0, None, 1, 3))
        if self.kind == "lgn":
            # user / item: dense gradients (they enter through concat), ONE norm over the whole summed gradient (slots 6 / 0),
            # no regulariser on the raw rows (slot None: it acts on F).  cate: the Vi slices of the item2cate lookup (slot 1)
            # plus the involved-rows slice, which is the usual regulariser term (its norm in slot 5); slot 3 stays zero
            # (the step applies cate's term itself, to the involved rows only: the table's flags also hold set(item2cate))
            return (("item", None, None, 0.0, 0.0, None, 0, 1), ("cate", None, None, 0.0, 0.0, None, 1, 3),
                    ("user", None, None, 0.0, 0.0, None, 6, 1))
        if self.kind != "ncf":
            return trunk
        # NCF: item / cate get the regulariser only (their lookup-site slots 0..3 stay zero); its own four tables have
        # one lookup site each (slots 6..9, written by the kernel from the un-merged slices) and no regulariser (slot None)
        return trunk + tuple((k, None, None, 0.0, 0.0, None, 6 + i, 1)
                             for i, k in enumerate(("user_gmf", "user_mlp", "item_gmf", "item_mlp")))

    def _att_qh(self, key):
        return 0

    def _det_merged(self, f):
        if self.kind in ("ncf", "lgn"):      # (no history lookup reaches the loss: nothing to merge)
            return {}
        if self.kind == "nextitnet":
            # the Hn T G target rows of a training step, ids in (h, t, g) order (clsr_nextitnet_rows; _nextitnet_forward
            # hangs the two id lists into the feed)
            n = f["B"] * f["T"]
            return {"item": ("nx_items_t", n), "cate": ("nx_cates_t", n)}
        return self._det_merged_hist(f)

    def _det_merged_hist(self, f):
        """As in the CLSR graph, the target rows' ids follow the history lookup's ids in ONE sorted list per table: no
        float atomics on the target site, two runs of a step give bit-identical gradient tables."""
        return {"item": ("items", f["B"]), "cate": ("cates", f["B"])}

    # ------------------------------------------------------------------ encoders
    def _gru_list(self):
        if self.kind == "gru4rec":
            return [("gs", self.sc["gru"], self.H)]
        if self.kind == "dien":
            return [("gs", self.sc["gru1"], self.H)]
        return []

    @property
    def _t4_kind(self):
        return "time4lstm" if self.kind == "sli_rec" else None

    @property
    def _t4_scope(self):
        return self.sc["t4"] if self.kind == "sli_rec" else None

    @property
    def a_in(self):
        return 3 * self.D + 1

    @property
    def out_dim(self):
        """Width of ``model_output`` (the logit MLP's input)."""
        if self.kind == "caser":
            return 2 * (int(self.hp.n_v) + int(self.hp.L) * int(self.hp.n_h)) + self.D
        if self.kind == "ncf":
            return self.nc_Du + int(self.hp.ncf_layer_sizes[-1])
        if self.kind in ("nextitnet", "sasrec"):
            return 2 * self.D
        return {"gru4rec": self.H + self.D, "din": 3 * self.D, "sli_rec": 2 * self.D, "a2svd": 2 * self.D,
                "dien": 3 * self.D + self.H}[self.kind]

    def _plan_weights(self, training):
        hp, P, D, H = self.hp, self.P, self.D, self.H
        pair = self._pack_pair if training else (lambda k, W, K, N, K_pad=None: self._pack(k, W, N, K, in_pad=K_pad))
        if self.kind == "din":
            self._plan_att("st", self.sc["att"], D, D, training)
        elif self.kind == "sli_rec":
            self._plan_att("st", self.sc["att"], H, D, training)
            pair("asvd.A", P[self.sc["asvd"] + "attention_mat"], D, D)
            if not hp.manual_alpha:
                a = self.sc["alpha"] + "nn_part/"
                pair("al.W0", P[a + "w_nn_layer0"], self.a_in, self.A0, K_pad=_pad4(self.a_in))
                pair("al.W1", P[a + "w_nn_layer1"], self.A0, self.A1)
        elif self.kind == "a2svd":
            pair("asvd.A", P[self.sc["asvd"] + "attention_mat"], D, D)
        elif self.kind == "dien":
            self._plan_att("st", self.sc["att"], H, D, training)
            # input side of the attentional GRU: [gates (2H) | candidate (H)] over the first GRU's outputs
            g2 = self.sc["gru2"]
            bias = self._buf("a2.bias", 3 * H)
            for W_, b_, off, w in ((P[g2 + "gates/kernel"][0:H], P[g2 + "gates/bias"], 0, 2 * H),
                                   (P[g2 + "candidate/kernel"][0:H], P[g2 + "candidate/bias"], 2 * H, H)):
                self._pack("a2.xw", W_, w, H, o0=off, total=(3 * H, H))
                self._cur_descs.append(ops.pack_desc(b_, w, 1, bias, 1, ld1=1, o0=off))
                if training:
                    self._pack("a2.xw^T", W_, H, w, transposed=True, i0=off, total=(H, 3 * H))
        if self.kind in ("gru4rec", "sli_rec", "dien"):
            self._plan_encoders(training)
        pair("lg.W0", P[LG + "w_nn_layer0"], self.out_dim, self.L0)
        pair("lg.W1", P[LG + "w_nn_layer1"], self.L0, self.L1)

    # ------------------------------------------------------------------ forward
    def _forward(self, f, training, after_attention=None, early_aux=None):
        if self.kind == "ncf":
            if training:
                raise ValueError("NCF's training forward is part of its step (clsr_ncf_train): use train_step")
            return self._ncf_score(f)
        if self.kind == "lgn":
            if training:
                raise ValueError("LGN's training forward is part of its step: use train_step")
            return self._lgn_score(f)
        if self.kind == "nextitnet":
            return self._nextitnet_forward(f, training, early_aux)
        hp, P, kind, sc = self.hp, self.P, self.kind, self.sc
        B, T = f["B"], f["T"]
        G = self.G_train if (training and self.dedup) else ((f.get("G") or 1) if not training else 1)
        if B % G:
            raise ValueError("training feed rows (%d) must be a multiple of 1+train_num_ngs (%d)" % (B, G))
        Hn = B // G
        D, H, Di, Dc, E = self.D, self.H, self.Di, self.Dc, self.enc_in
        self.last_shape = (B, T, G, Hn)
        self._pack_all(training)
        hs = 1 if f.get("compact") else G
        seq_len, ls = f["seq_len"], hs
        step_start = self._fork_point()
        # ---- gathers (padded steps hold embedding row 0, as in the reference)
        hist = self._buf("hist", Hn, T, D)
        hmean, hrec = self._buf("hist_mean", Hn, D), self._buf("hist_recent", Hn, D)
        call("clsr_gather_hist_fwd", self.tables["item"], self.tables["cate"], f["item_history"],
             f["item_cate_history"], hs * T, seq_len, ls, Hn, T, Di, Dc, 1, hist, hmean, hrec)
        target = self._buf("target", B, D)
        tb = self.tables
        ops.multi("clsr_gather_rows_multi", ops.GatherDesc, [
            ops.GatherDesc.row(table=tb["item"], idx=f["items"], out=target, idx_stride=1, N=B, C=Di, ldo=D),
            ops.GatherDesc.row(table=tb["cate"], idx=f["cates"], out=target, idx_stride=1, N=B, C=Dc, ldo=D, col0=Di)])
        M = Hn * T
        W = self.out_dim
        mo = self._buf("model_output", B, W)
        out = dict(hist_input=hist, target=target, model_output=mo)

        def aux():
            if early_aux is not None or training:
                with self._branch("@aux", after=step_start):
                    if early_aux is not None:
                        early_aux()
                    if training:
                        self._sort_hist_ids(f, Hn, T, hs)

        if kind == "gru4rec":
            NX = self.NX
            PinAll = self._buf("xw.Pin", M, NX)
            self._gemm(hist, D, "xw", M, E, NX, PinAll, NX, bias=self._buf("xw.bias", NX))
            aux()
            d, hT, _ = self._gru_fwd_desc("gs", sc["gru"], H, PinAll, Hn, T, None, training)
            ops.rnn_multi("clsr_rnn_fwd_multi", [d], None, seq_len, ls, Hn, T)
            call("clsr_copy_cols", hT, H, 0, G, B, H, mo, W, 0, 0)
            call("clsr_copy_cols", target, D, 0, 1, B, D, mo, W, H, 0)
            out["final_state"] = hT
        elif kind == "dien":
            NX = self.NX
            PinAll = self._buf("xw.Pin", M, NX)
            self._gemm(hist, D, "xw", M, E, NX, PinAll, NX, bias=self._buf("xw.bias", NX))
            aux()
            d1, _, rnn1 = self._gru_fwd_desc("gs", sc["gru1"], H, PinAll, Hn, T, None, training, want_seq=True)
            ops.rnn_multi("clsr_rnn_fwd_multi", [d1], None, seq_len, ls, Hn, T)
            hsum = self._buf("hist_sum", Hn, D)
            call("clsr_scale_rows_by_len", hmean, seq_len, ls, Hn, D, hsum, 0)
            # attention over the first GRU's outputs: only its WEIGHTS are used (return_alpha=True)
            self._att_fwd("st", sc["att"], rnn1, target, Hn, G, T, H, D, seq_len, ls, training)
            wts = self._buf("st.wts", B, T)
            # attentional GRU: one sequence per candidate row, inputs shared by the rows of a history group
            g2 = sc["gru2"]
            Pin2 = self._buf("a2.Pin", M, 3 * H)
            self._gemm(rnn1, H, "a2.xw", M, H, 3 * H, Pin2, 3 * H, bias=self._buf("a2.bias", 3 * H))
            hT2 = self._buf("a2.hT", B, H)
            d2 = ops.gru_desc(H, Pin=Pin2, ldp=3 * H, Wgh=P[g2 + "gates/kernel"][H:], ldg=2 * H,
                              Wch=P[g2 + "candidate/kernel"][H:], ldc=H, hT=hT2,
                              hprev=self._buf("a2.hprev", B, T, H) if training else None,
                              gates=self._buf("a2.gates", B, T, 3 * H) if training else None, att=wts, in_div=G)
            ops.rnn_multi("clsr_rnn_fwd_multi", [d2], None, seq_len, ls, B, T)
            call("clsr_copy_cols", target, D, 0, 1, B, D, mo, W, 0, 0)
            call("clsr_copy_cols", hT2, H, 0, 1, B, H, mo, W, D, 0)
            call("clsr_copy_cols", hsum, D, 0, G, B, D, mo, W, D + H, 0)
            call("clsr_mul_rows", target, D, hsum, D, G, B, D, mo[:, 2 * D + H:], W)
            out.update(hist_sum=hsum, rnn_out=rnn1, w_att=wts, final_state=hT2)
        elif kind == "a2svd":
            ai = self._buf("asvd.ai", M, D)
            self._gemm(hist, D, "asvd.A", M, D, D, ai, D)
            aux()
            w1, att1 = self._buf("asvd.wts", Hn, T), self._buf("asvd.out", Hn, D)
            call("clsr_asvd_att_fwd", ai, P[sc["asvd"] + "query"], hist, Hn, T, D, w1, att1)
            call("clsr_copy_cols", att1, D, 0, G, B, D, mo, W, 0, 0)
            call("clsr_copy_cols", target, D, 0, 1, B, D, mo, W, D, 0)
            out.update(asvd_output=att1, w_asvd=w1)
        elif kind == "din":
            hsum = self._buf("hist_sum", Hn, D)
            call("clsr_scale_rows_by_len", hmean, seq_len, ls, Hn, D, hsum, 0)
            aux()
            att = self._att_fwd("st", sc["att"], hist, target, Hn, G, T, D, D, seq_len, ls, training)
            call("clsr_copy_cols", target, D, 0, 1, B, D, mo, W, 0, 0)
            call("clsr_copy_cols", hsum, D, 0, G, B, D, mo, W, D, 0)
            call("clsr_copy_cols", att, D, 0, 1, B, D, mo, W, 2 * D, 0)
            out.update(hist_sum=hsum, att_fea=att, w_att=self._buf("st.wts", B, T))
        elif kind == "caser":
            if T != self.cz_T:
                raise ValueError("Caser's vertical kernels are [Dx, max_seq_length, n_v]: the feed must hold "
                                 "max_seq_length = %d steps, got %d" % (self.cz_T, T))
            aux()
            PW2 = 2 * self.cz_pw
            pooled = self._buf("cz.pooled", Hn, PW2)
            am = [self._buf("cz.argmax." + k, Hn, self.cz_L, self.cz_nh, dtype=torch.int32) for k in ("item", "cate")]
            # per pool: number of positions tied with the maximum | their bit mask (the backward splits evenly, as TF does)
            ti = [self._buf("cz.ties." + k, Hn, self.cz_L, self.cz_nh, 1 + (T + 31) // 32, dtype=torch.int32)
                  for k in ("item", "cate")]
            call("clsr_caser_hconv_fwd", hist, D, Hn, T, Di, Dc, self.cz_W["item"], self.cz_W["cate"], self.cz_L,
                 self.cz_nv, self.cz_nh, pooled, PW2, am[0], am[1], ti[0], ti[1])
            call("clsr_copy_cols", pooled, PW2, 0, G, B, PW2, mo, W, 0, 0)
            call("clsr_copy_cols", target, D, 0, 1, B, D, mo, W, PW2, 0)
            out.update(pooled=pooled, argmax_item=am[0], argmax_cate=am[1], ties_item=ti[0], ties_cate=ti[1])
        elif kind == "sasrec":
            if T > self.sa_T:
                raise ValueError("SASRec's positional table holds max_seq_length = %d rows: the feed holds %d steps"
                                 % (self.sa_T, T))
            aux()
            # ONE launch for the whole stack; training saves every block's input and the last valid row, scoring nothing.
            # s lands in columns 0 .. D of all G rows of its history group
            saved = self._buf("sa.saved", query("clsr_sasrec_saved_floats", Hn, T, D, self.sa_nb)) if training else None
            tile = self._sasrec_tile(T)
            if tile:
                # a shape the resident kernels refuse: the tiled pair, its workspace sized for this launch (training: the
                # backward's partial sums and parked rows, which the backward of this step fetches under the same name)
                ws = self._buf("sa.tws.train" if training else "sa.tws.score",
                               query("clsr_sasrec_tiled_workspace_floats", Hn, T, self.sa_T, D, self.sa_nb, tile, int(training)))
                call("clsr_sasrec_tiled_fwd", hist, seq_len, ls, Hn, T, self.sa_T, D, self.sa_W, self.sa_nb, self.sa_nh, saved,
                     mo, W, G, tile, ws)
            else:
                call("clsr_sasrec_fwd", hist, seq_len, ls, Hn, T, self.sa_T, D, self.sa_W, self.sa_nb, self.sa_nh, saved, mo,
                     W, G)
            call("clsr_copy_cols", target, D, 0, 1, B, D, mo, W, D, 0)
            out.update(saved=saved)
        else:
            NX = self.NX
            t = sc["t4"]
            # long-term: A2SVD attention over the whole (padded) history
            ai = self._buf("asvd.ai", M, D)
            self._gemm(hist, D, "asvd.A", M, D, D, ai, D)
            w1, att1 = self._buf("asvd.wts", Hn, T), self._buf("asvd.out", Hn, D)
            call("clsr_asvd_att_fwd", ai, P[sc["asvd"] + "query"], hist, Hn, T, D, w1, att1)
            # short-term: Time4LSTM over [item embedding | t_first | t_now], then attention_fcn(target, outputs)
            TT = self._buf("t4.TT", M, 2 * H)
            call("clsr_t4_time_inputs_fwd", f["time_to_now"], f["time_from_first_action"], hs * T,
                 P[t + "_time_input_w1"], P[t + "_time_input_bias1"], P[t + "_time_input_w2"],
                 P[t + "_time_input_bias2"], Hn, T, H, TT)
            PinAll = self._buf("xw.Pin", M, NX)
            self._gemm(hist, D, "xw", M, E, NX, PinAll, NX, bias=self._buf("xw.bias", NX))
            aux()
            t4off = self._enc_off("t4")
            self._gemm(TT, 2 * H, "t4.tw", M, 2 * H, 3 * H, PinAll[:, t4off + 3 * H:], NX, acc=1)
            rnn_out = self._buf("rnn_out", Hn, T, H)
            t4d = ops.t4_desc(H, Pin=PinAll[:, t4off:], ldp=NX, Wm=P[t + "kernel"][E:], ldm=4 * H, out_seq=rnn_out,
                              act=self._buf("t4.act", Hn, T, 6 * H) if training else None,
                              cst=self._buf("t4.cst", Hn, T, H) if training else None,
                              mprev=self._buf("t4.mprev", Hn, T, H) if training else None)
            ops.rnn_multi("clsr_rnn_fwd_multi", [], t4d, seq_len, ls, Hn, T)
            att2 = self._att_fwd("st", sc["att"], rnn_out, target, Hn, G, T, H, D, seq_len, ls, training)
            alpha = self._buf("alpha", B)
            if not hp.manual_alpha:
                ld = _pad4(self.a_in)
                ain = self._buf("al.in", B, ld)
                call("clsr_alpha_concat", None, 0, target, att1, att2, f["time_to_now"], T, T - 1,
                     G if f.get("compact") else 1, B, G, D, ain, ld)
                al_logit = self._mlp_fwd("al", sc["alpha"] + "nn_part/", ain, ld, ld, (self.A0, self.A1), B, training)
                call("clsr_alpha_fuse_fwd", al_logit, 0.0, att1, att2, target, B, G, D, alpha, mo)
            else:
                call("clsr_alpha_fuse_fwd", None, float(hp.manual_alpha_value), att1, att2, target, B, G, D, alpha, mo)
            out.update(att_fea1=att1, att_fea2=att2, rnn_out=rnn_out, alpha=alpha, w_asvd=w1,
                       w_att=self._buf("st.wts", B, T))
        self._join()
        if training and self.drop_on:
            out["logit"] = self._mlp_fwd_drop("lg", LG, mo, W, W, (self.L0, self.L1), B)
        else:       # (evaluation and predict never drop: keep_prob_test)
            out["logit"] = self._mlp_fwd("lg", LG, mo, W, W, (self.L0, self.L1), B, training)
        return out

    # ------------------------------------------------------------------ training step
    def _train_step(self, f, apply):
        if self.kind == "ncf":
            return self._ncf_train_step(f, apply)
        if self.kind == "lgn":
            return self._lgn_train_step(f, apply)
        if self.kind == "nextitnet":
            return self._nextitnet_train_step(f, apply)
        hp, P, Gd, kind, sc = self.hp, self.P, self.Gd, self.kind, self.sc
        self._step = _StepState(f)     # (these graphs set none of its other fields: the shared phases read idle ones)
        if self.drop_on:
            call("clsr_dropout_tick", self.drop_state)     # first launch of the step: this step's draw number
        B, T = f["B"], f["T"]
        G = self.G_train if self.dedup else 1
        Hn = B // G
        D, H, Di, Dc, E = self.D, self.H, self.Di, self.Dc, self.enc_in
        hs = 1 if f.get("compact") else G
        seq_len, ls = f["seq_len"], hs
        M, W = Hn * T, self.out_dim
        zpool = self._buf("zero_pool", M * (D + H) + B * D * 3 + Hn * (3 * D + H) + B * T)
        fl = self.tab_flags

        def zero_and_mark():
            call("clsr_zero_doubles", self.losses, 8)
            call("clsr_zero_doubles", self.sumsq_tab, 16)
            call("clsr_zero_floats", zpool, zpool.numel())
            mark = ops.MarkDesc.row
            ops.multi("clsr_mark_rows_multi", ops.MarkDesc, [
                mark(idx=f["item_history"], flags=fl["item"], nrows=Hn, row_stride=hs * T, ncols=T),
                mark(idx=f["items"], flags=fl["item"], nrows=B, row_stride=1, ncols=1),
                mark(idx=f["item_cate_history"], flags=fl["cate"], nrows=Hn, row_stride=hs * T, ncols=T),
                mark(idx=f["cates"], flags=fl["cate"], nrows=B, row_stride=1, ncols=1)])
        take = self._carver(zpool)
        dhist, drnn = take(Hn, T, D), take(Hn, T, H)
        dtarget, dS, datt = take(B, D), take(B, D), take(B, D)
        dL, dM, dR, dhT = take(Hn, D), take(Hn, D), take(Hn, D), take(Hn, H)
        dwts = take(B, T)      # DIEN: gradient w.r.t. the attention WEIGHTS (datt is d att_fea, [B, D])
        out = self._forward(f, True, None, zero_and_mark)
        dlogit = self._buf("dlogit", B)
        Gl = hp.train_num_ngs + 1
        call("clsr_softmax_loss", out["logit"], f["labels"], B // Gl, Gl, 1.0 / ((B // Gl) * self.dp_world),
             self.losses[0:], dlogit)
        mlp_bwd = self._mlp_bwd_drop if self.drop_on else self._mlp_bwd
        dmo = mlp_bwd("lg", LG, dlogit, out["model_output"], W, W, W, (self.L0, self.L1), B)
        hist = out["hist_input"]
        if kind == "gru4rec":
            NX = self.NX
            call("clsr_group_sum_cols", dmo, W, 0, G, Hn, H, dhT, H, 0, 1)
            call("clsr_copy_cols", dmo, W, H, 1, B, D, dtarget, D, 0, 1)
            dPinAll = self._buf("xw.dPin", M, NX)
            ops.rnn_multi("clsr_rnn_bwd_multi", [self._gru_bwd_desc("gs", sc["gru"], H, dPinAll, Hn, T, dhT, None,
                                                                     None)], None, seq_len, ls, Hn, T)
            self._enc_input_bwd(hist, dPinAll, dhist, M)
            self._gru_bwd_hidden("gs", sc["gru"], H, dPinAll, Hn, T)
            self._dw_flush()
            self._unpack_grads()
        elif kind == "dien":
            NX = self.NX
            g2 = sc["gru2"]
            rnn1, wts, target, hsum = out["rnn_out"], out["w_att"], out["target"], out["hist_sum"]
            call("clsr_copy_cols", dmo, W, 0, 1, B, D, dtarget, D, 0, 1)
            dhT2 = self._buf("a2.dhT", B, H)
            call("clsr_copy_cols", dmo, W, D, 1, B, H, dhT2, H, 0, 0)
            dsum = self._buf("d_hist_sum", Hn, D)
            call("clsr_group_sum_cols", dmo, W, D + H, G, Hn, D, dsum, D, 0, 0)
            # product feature target * hist_sum: d target += dp * hist_sum[h], d hist_sum[h] += sum_g dp * target
            dsum2 = self._buf("d_hist_sum2", Hn, D)
            call("clsr_att_prod_bwd_ld", dmo[:, 2 * D + H:], W, hsum, D, target, D, Hn, G, 1, D, dsum2, D, dtarget, D, 1)
            call("clsr_axpby", dsum, dsum, 1.0, dsum2, 1.0, Hn * D)
            call("clsr_scale_rows_by_len", dsum, seq_len, ls, Hn, D, dM, 0)
            # attentional GRU backward (row level): d att scores, d input projections per row
            dPin2 = self._buf("a2.dPin", B * T, 3 * H)
            hprev2, gates2 = self._buf("a2.hprev", B, T, H), self._buf("a2.gates", B, T, 3 * H)
            d2 = ops.gru_desc(H, Wgh=P[g2 + "gates/kernel"][H:], ldg=2 * H, Wch=P[g2 + "candidate/kernel"][H:], ldc=H,
                              hprev=hprev2, gates=gates2, dhT=dhT2, dPin=dPin2, lddp=3 * H, att=wts, datt=dwts,
                              in_div=G)
            ops.rnn_multi("clsr_rnn_bwd_multi", [d2], None, seq_len, ls, B, T)
            self._dw(hprev2, H, dPin2, 3 * H, B * T, H, 2 * H, Gd[g2 + "gates/kernel"][H:], 2 * H)
            self._dw(hprev2, H, dPin2[:, 2 * H:], 3 * H, B * T, H, H, Gd[g2 + "candidate/kernel"][H:], H, Xmul=gates2,
                     ldmul=3 * H)
            if G > 1:       # the rows of a group share the inputs: sum their d(input projections)
                # (as 3 T steps of H columns -- the same memory, the same sums over the group's rows: the kernel takes at
                # most 256 columns, and 3 H passes that from hidden_size 88 on)
                dPin2h = self._buf("a2.dPinH", M, 3 * H)
                call("clsr_att_z0_bwd_reduce", dPin2, Hn, G, 3 * T, H, dPin2h, self._buf("a2.dV", B, 3 * H))
            else:
                dPin2h = dPin2
            self._dw(rnn1, H, dPin2h, 3 * H, M, H, 2 * H, Gd[g2 + "gates/kernel"][0:H], 2 * H,
                     db=Gd[g2 + "gates/bias"])
            self._dw(rnn1, H, dPin2h[:, 2 * H:], 3 * H, M, H, H, Gd[g2 + "candidate/kernel"][0:H], H,
                     db=Gd[g2 + "candidate/bias"])
            self._gemm(dPin2h, 3 * H, "a2.xw^T", M, 3 * H, H, drnn, H, acc=1)
            # attention backward through its weights, then the first GRU
            dq = self._att_bwd("st", sc["att"], None, rnn1, target, drnn, Hn, G, T, H, D, seq_len, ls, dw_in=dwts)
            call("clsr_copy_cols", dq, D, 0, 1, B, D, dtarget, D, 0, 1)
            dPinAll = self._buf("xw.dPin", M, NX)
            ops.rnn_multi("clsr_rnn_bwd_multi", [self._gru_bwd_desc("gs", sc["gru1"], H, dPinAll, Hn, T, None, drnn,
                                                                     None)], None, seq_len, ls, Hn, T)
            self._enc_input_bwd(hist, dPinAll, dhist, M)
            self._gru_bwd_hidden("gs", sc["gru1"], H, dPinAll, Hn, T)
            self._dw_flush()
            self._unpack_grads()
        elif kind == "a2svd":
            call("clsr_group_sum_cols", dmo, W, 0, G, Hn, D, dL, D, 0, 1)
            call("clsr_copy_cols", dmo, W, D, 1, B, D, dtarget, D, 0, 1)
            self._asvd_bwd(dL, hist, dhist, Hn, T)
            self._dw_flush()
        elif kind == "din":
            call("clsr_copy_cols", dmo, W, 0, 1, B, D, dtarget, D, 0, 1)
            dsum = self._buf("d_hist_sum", Hn, D)
            call("clsr_group_sum_cols", dmo, W, D, G, Hn, D, dsum, D, 0, 0)
            call("clsr_copy_cols", dmo, W, 2 * D, 1, B, D, datt, D, 0, 0)
            dq = self._att_bwd("st", sc["att"], datt, hist, out["target"], dhist, Hn, G, T, D, D, seq_len, ls)
            call("clsr_copy_cols", dq, D, 0, 1, B, D, dtarget, D, 0, 1)
            # d(masked sum) reaches every valid step: hand it to the embedding backward as len * d(mean)
            call("clsr_scale_rows_by_len", dsum, seq_len, ls, Hn, D, dM, 0)
            self._dw_flush()
        elif kind == "caser":
            PW2 = 2 * self.cz_pw
            dpool = self._buf("cz.dpool", Hn, PW2)
            call("clsr_group_sum_cols", dmo, W, 0, G, Hn, PW2, dpool, PW2, 0, 0)
            call("clsr_copy_cols", dmo, W, PW2, 1, B, D, dtarget, D, 0, 1)
            shape = (Hn, T, Di, Dc, self.cz_L, self.cz_nv, self.cz_nh)
            ws = self._buf("cz.ws", query("clsr_caser_hconv_bwd_workspace_floats", *shape))
            # d hist of both paths (padded steps included: their rows reach table row 0) and every kernel / bias gradient
            call("clsr_caser_hconv_bwd", dpool, PW2, out["pooled"], PW2, out["argmax_item"], out["argmax_cate"],
                 out["ties_item"], out["ties_cate"], hist, D, Hn, T, Di, Dc, self.cz_W["item"], self.cz_W["cate"],
                 self.cz_L, self.cz_nv, self.cz_nh, dhist, self.cz_dW["item"], self.cz_dW["cate"], ws)
            self._dw_flush()
        elif kind == "sasrec":
            call("clsr_group_sum_cols", dmo, W, 0, G, Hn, D, dL, D, 0, 1)
            call("clsr_copy_cols", dmo, W, D, 1, B, D, dtarget, D, 0, 1)
            shape = (Hn, T, self.sa_T, D, self.sa_nb)
            tile = self._sasrec_tile(T)
            # ONE launch: d hist is written (padded steps: 0.0), every dense gradient leaves as a row of sums per workgroup
            if tile:
                parts = query("clsr_sasrec_tiled_parts", *shape)
                ws = self._buf("sa.tws.train", query("clsr_sasrec_tiled_workspace_floats", *(shape + (tile, 1))))
                call("clsr_sasrec_tiled_bwd", dL, out["saved"], seq_len, ls, Hn, T, self.sa_T, D, self.sa_W, self.sa_nb,
                     self.sa_nh, dhist, tile, ws)
            else:
                parts = query("clsr_sasrec_parts", *shape)
                ws = self._buf("sa.ws", query("clsr_sasrec_workspace_floats", *shape))
                call("clsr_sasrec_bwd", dL, out["saved"], seq_len, ls, Hn, T, self.sa_T, D, self.sa_W, self.sa_nb, self.sa_nh,
                     dhist, ws)
            self._rp(ws, parts, self.sa_P, self.sa_P, self.sa_dW)
            self._dw_flush()
        else:
            NX = self.NX
            t = sc["t4"]
            att1, att2 = out["att_fea1"], out["att_fea2"]
            if not hp.manual_alpha:
                dal = self._buf("dalpha_logit", B)
                call("clsr_alpha_fuse_bwd", dmo, out["alpha"], 0.0, att1, att2, Hn, G, D, dal, dL, dS, dtarget)
                ld = _pad4(self.a_in)
                dain = self._mlp_bwd("al", sc["alpha"] + "nn_part/", dal, self._buf("al.in", B, ld), ld, ld, self.a_in,
                                     (self.A0, self.A1), B)
                call("clsr_alpha_concat_bwd", dain, ld, 0, Hn, G, D, None, dtarget, dL, dS)
            else:
                call("clsr_alpha_fuse_bwd", dmo, None, float(hp.manual_alpha_value), att1, att2, Hn, G, D, None, dL,
                     dS, dtarget)
            dq = self._att_bwd("st", sc["att"], dS, out["rnn_out"], out["target"], drnn, Hn, G, T, H, D, seq_len, ls)
            call("clsr_copy_cols", dq, D, 0, 1, B, D, dtarget, D, 0, 1)
            dPinAll = self._buf("xw.dPin", M, NX)
            t4off = self._enc_off("t4")
            t4d = ops.t4_desc(H, Wm=P[t + "kernel"][E:], ldm=4 * H, act=self._buf("t4.act", Hn, T, 6 * H),
                              cst=self._buf("t4.cst", Hn, T, H), dout_seq=drnn, dPin=dPinAll[:, t4off:], lddp=NX)
            ops.rnn_multi("clsr_rnn_bwd_multi", [], t4d, seq_len, ls, Hn, T)
            self._enc_input_bwd(hist, dPinAll, dhist, M)
            self._t4_bwd_weights(f, dPinAll, Hn, T, hs)
            self._asvd_bwd(dL, hist, dhist, Hn, T)
            self._dw_flush()
            self._unpack_grads()
        self._join()
        # ---- embedding gradients
        ss = self.sumsq_tab
        if self.det_grads and self._det_merged(f):
            # the target rows ride in the sorted lists of the history lookups: every gradient row summed in a fixed order
            self._hist_grad_sorted(dhist, dM, dR, Hn, T, seq_len, ls, ss, dtarget=dtarget)
        else:
            self._hist_grad_sorted(dhist, dM, dR, Hn, T, seq_len, ls, ss)
            call("clsr_scatter_add_rows", dtarget, D, 0, f["items"], 1, B, Di, self.tab_grad["item"], ss[2:])
            call("clsr_scatter_add_rows", dtarget, D, Di, f["cates"], 1, B, Dc, self.tab_grad["cate"], ss[3:])
        if apply:
            self._apply_updates()
        return out

    # ------------------------------------------------------------------ NCF
    def _ncf_tables(self):
        tb = self.tables
        return tb["user_gmf"], tb["user_mlp"], tb["item_gmf"], tb["item_mlp"]

    def _ncf_score(self, f):
        """Evaluation / predict: ONE launch from the ids to the logits (no history gather: nothing reads it)."""
        B, T = f["B"], f["T"]
        G = ((f.get("G") or 1) if self.dedup else 1) if f.get("compact") else 1
        if B % G:
            raise ValueError("feed rows (%d) must be a multiple of the history group (%d)" % (B, G))
        self.last_shape = (B, T, G, B // G)
        logit, mo = self._buf("logit", B), self._buf("model_output", B, self.out_dim)
        # (a compact feed holds one user per group of G lines; the gathers are per line all the same)
        call("clsr_ncf_score", f["users"], G, f["items"], *self._ncf_tables(), self.nc_W, self.nc_Du, self.nc_nl,
             *self.nc_w4, B, logit, mo)
        return dict(logit=logit, model_output=mo)

    def _ncf_train_step(self, f, apply):
        """Marks, the two launches of clsr_ncf_train, then the shared phases: the partial-sum reduction of the dense
        gradients, the table-gradient path over the four slice buffers, regulariser + clip + optimiser."""
        hp = self.hp
        self._step = _StepState(f)
        B, T = f["B"], f["T"]
        G = self.G_train if self.dedup else 1
        Gl = hp.train_num_ngs + 1
        if B % Gl:
            raise ValueError("training feed rows (%d) must be a multiple of 1+train_num_ngs (%d)" % (B, Gl))
        Hn = B // G
        hs = 1 if f.get("compact") else G
        udiv = G if f.get("compact") else 1        # lines per entry of f["users"]
        self.last_shape = (B, T, G, Hn)
        Du, W, fl = self.nc_Du, self.out_dim, self.tab_flags
        call("clsr_zero_doubles", self.losses, 8)
        call("clsr_zero_doubles", self.sumsq_tab, 16)
        # involved rows: item / cate as in every model of the trunk (their regulariser), the four NCF tables' touched rows
        mark = ops.MarkDesc.row
        ops.multi("clsr_mark_rows_multi", ops.MarkDesc, [
            mark(idx=f["item_history"], flags=fl["item"], nrows=Hn, row_stride=hs * T, ncols=T),
            mark(idx=f["items"], flags=fl["item"], nrows=B, row_stride=1, ncols=1),
            mark(idx=f["item_cate_history"], flags=fl["cate"], nrows=Hn, row_stride=hs * T, ncols=T),
            mark(idx=f["cates"], flags=fl["cate"], nrows=B, row_stride=1, ncols=1),
            mark(idx=f["users"], flags=fl["user_gmf"], nrows=B // udiv, row_stride=1, ncols=1),
            mark(idx=f["users"], flags=fl["user_mlp"], nrows=B // udiv, row_stride=1, ncols=1),
            mark(idx=f["items"], flags=fl["item_gmf"], nrows=B, row_stride=1, ncols=1),
            mark(idx=f["items"], flags=fl["item_mlp"], nrows=B, row_stride=1, ncols=1)])
        logit, mo, dlogit = self._buf("logit", B), self._buf("model_output", B, W), self._buf("dlogit", B)
        keys = ("user_gmf", "user_mlp", "item_gmf", "item_mlp")
        sl = [self._buf("nc.d_" + k, B, Du) for k in keys]
        uid = self._buf("nc.uid", B, dtype=torch.int32)
        shape = (self.nc_Du, self.nc_nl) + self.nc_w4
        parts = query("clsr_ncf_parts", B, Gl)
        ws = self._buf("nc.ws", query("clsr_ncf_workspace_floats", B, Gl, *shape))
        ss = self.sumsq_tab
        call("clsr_ncf_train", f["users"], udiv, f["items"], f["labels"], *self._ncf_tables(), self.nc_W, *shape, B, Gl,
             1.0 / ((B // Gl) * self.dp_world), logit, mo, dlogit, sl[0], sl[1], sl[2], sl[3], uid, ws, self.losses[0:],
             ss[6:])
        self._rp(ws[10 * parts:], parts, self.nc_P, self.nc_P, self.nc_dW)
        self._dw_flush()
        # ---- the slices reach the gradient tables (their squared norms are in slots 6..9 already: taken from the slices)
        tg = self.tab_grad
        ids = (uid, uid, f["items"], f["items"])
        if self.det_grads:
            sort = []
            for name, idx, V in (("ncf_user", uid, self.dims["Vu"]), ("ncf_item", f["items"], self.dims["Vi"])):
                sort.append(ops.SortIdsDesc.row(
                    ids=idx, keys_out=self._buf("sort.keys." + name, B, dtype=torch.int32),
                    perm_out=self._buf("sort.perm." + name, B, dtype=torch.int32), nrows=B, row_stride=1, ncols=1,
                    bits=max(1, (V - 1).bit_length())))
            sws = self._buf("sort.ws", query("clsr_sort_ids_stable_workspace_bytes", 2 * B, 2), dtype=torch.uint8)
            ops.sort_ids_stable_multi(sort, sws)
            self._segsum("ncf", [self._site_row("ncf_" + k.split("_")[0], s, Du, 0, Du, B, tg[k], None)
                                 for k, s in zip(keys, sl)])
        else:
            for k, s, idx in zip(keys, sl, ids):
                call("clsr_scatter_add_rows", s, Du, 0, idx, 1, B, Du, tg[k], None)
        out = dict(logit=logit, model_output=mo, dlogit=dlogit, slices=dict(zip(keys, sl)))
        if apply:
            self._apply_updates()
        return out

    # ------------------------------------------------------------------ LGN
    def _lgn_node_table(self):
        """E_0 = [user_embedding ; item_embedding ++ cate_embedding[item2cate]]: three row gathers, one launch."""
        Vu, Vi, C, Di, Dc, tb = self.dims["Vu"], self.dims["Vi"], self.D, self.Di, self.Dc, self.tables
        E0 = self._buf("lg.E0", Vu + Vi, C)
        row = ops.GatherDesc.row
        ops.multi("clsr_gather_rows_multi", ops.GatherDesc, [
            row(table=tb["user"], idx=self.lg_all_users, out=E0, idx_stride=1, N=Vu, C=C, ldo=C),
            row(table=tb["item"], idx=self.lg_all_items, out=E0[Vu:], idx_stride=1, N=Vi, C=Di, ldo=C),
            row(table=tb["cate"], idx=self.lg_i2c, out=E0[Vu:], idx_stride=1, N=Vi, C=Dc, ldo=C, col0=Di)])
        return E0

    # F depends on the parameters only: evaluation propagates ONCE after the parameters changed (a training step,
    # load_state_dict), outside the recorded launch sequence of a batch, which is then the scoring launch alone
    def forward(self, f, training, after_attention=None, early_aux=None):
        if self.kind == "lgn" and not training and not self.lg_F_valid:
            with ops.stream_scope():
                self.lg_F = self.lg_prop.forward(self._lgn_node_table(), self.lg_W, self.lg_b, training=False)
            self.lg_F_valid = True
        return super(SeqNet, self).forward(f, training, after_attention, early_aux)

    def train_step(self, f, apply=True):
        if self.kind == "lgn":
            self.lg_F_valid = False
        return super(SeqNet, self).train_step(f, apply)

    def load_state_dict(self, sd, strict=True):
        if self.kind == "lgn":
            self.lg_F_valid = False
        return super(SeqNet, self).load_state_dict(sd, strict=strict)

    def _lgn_score(self, f):
        """Evaluation / predict: ONE launch from the ids to the logits, over the cached F."""
        B, T = f["B"], f["T"]
        G = ((f.get("G") or 1) if self.dedup else 1) if f.get("compact") else 1
        if B % G:
            raise ValueError("feed rows (%d) must be a multiple of the history group (%d)" % (B, G))
        self.last_shape = (B, T, G, B // G)
        logit = self._buf("logit", B)
        call("clsr_lgn_score", f["users"], G, f["items"], self.lg_F, self.dims["Vu"], self.dims["Vi"], self.D, B, logit)
        return dict(logit=logit)

    def _lgn_train_step(self, f, apply):
        """Marks and the node table, two propagation launches, scoring + group softmax, the logit backward's rows summed
        per id in sorted order into a zeroed dF, the regulariser on F's involved item rows, the propagation backward over the
        transposed graph, dE_0 split into the three table gradients with their norms, then the shared update phase."""
        hp = self.hp
        self._step = _StepState(f)
        B, T = f["B"], f["T"]
        G = self.G_train if self.dedup else 1
        Gl = hp.train_num_ngs + 1
        if B % Gl:
            raise ValueError("training feed rows (%d) must be a multiple of 1+train_num_ngs (%d)" % (B, Gl))
        Hn = B // G
        hs = 1 if f.get("compact") else G
        udiv = G if f.get("compact") else 1        # lines per entry of f["users"]
        self.last_shape = (B, T, G, Hn)
        Vu, Vi, C, Di, Dc = self.dims["Vu"], self.dims["Vi"], self.D, self.Di, self.Dc
        N, fl, prop, ss = Vu + Vi, self.tab_flags, self.lg_prop, self.sumsq_tab
        dF = self._buf("lg.dF", N, C)
        call("clsr_zero_doubles", self.losses, 8)
        call("clsr_zero_doubles", ss, 16)
        call("clsr_zero_floats", dF, dF.numel())
        call("clsr_zero_floats", self.lg_inv_all.view(torch.float32), self.lg_inv_all.numel() // 4)
        # rows an update visits: every row of the two dense-gradient tables; cate: set(item2cate) | involved.  lg_inv: the
        # involved items (history ids included), whose rows of F the regulariser reaches
        mark = ops.MarkDesc.row
        ops.multi("clsr_mark_rows_multi", ops.MarkDesc, [
            mark(idx=f["item_history"], flags=self.lg_inv, nrows=Hn, row_stride=hs * T, ncols=T),
            mark(idx=f["items"], flags=self.lg_inv, nrows=B, row_stride=1, ncols=1),
            mark(idx=f["item_cate_history"], flags=fl["cate"], nrows=Hn, row_stride=hs * T, ncols=T),
            mark(idx=f["cates"], flags=fl["cate"], nrows=B, row_stride=1, ncols=1),
            mark(idx=f["item_cate_history"], flags=self.lg_inv_c, nrows=Hn, row_stride=hs * T, ncols=T),
            mark(idx=f["cates"], flags=self.lg_inv_c, nrows=B, row_stride=1, ncols=1),
            mark(idx=self.lg_i2c, flags=fl["cate"], nrows=Vi, row_stride=1, ncols=1),
            mark(idx=self.lg_all_items, flags=fl["item"], nrows=Vi, row_stride=1, ncols=1),
            mark(idx=self.lg_all_users, flags=fl["user"], nrows=Vu, row_stride=1, ncols=1)])
        F = prop.forward(self._lgn_node_table(), self.lg_W, self.lg_b, training=True)
        logit, dlogit = self._buf("logit", B), self._buf("dlogit", B)
        call("clsr_lgn_score", f["users"], udiv, f["items"], F, Vu, Vi, C, B, logit)
        call("clsr_softmax_loss", logit, f["labels"], B // Gl, Gl, 1.0 / ((B // Gl) * self.dp_world), self.losses[0:], dlogit)
        du, di = self._buf("lg.d_user", B, C), self._buf("lg.d_item", B, C)
        uid = self._buf("lg.uid", B, dtype=torch.int32)
        call("clsr_lgn_logit_bwd", f["users"], udiv, f["items"], F, Vu, Vi, C, B, dlogit, du, di, uid)
        sort = []
        for name, idx, V in (("lgn_user", uid, Vu), ("lgn_item", f["items"], Vi)):
            sort.append(ops.SortIdsDesc.row(
                ids=idx, keys_out=self._buf("sort.keys." + name, B, dtype=torch.int32),
                perm_out=self._buf("sort.perm." + name, B, dtype=torch.int32), nrows=B, row_stride=1, ncols=1,
                bits=max(1, (V - 1).bit_length())))
        sws = self._buf("sort.ws", query("clsr_sort_ids_stable_workspace_bytes", 2 * B, 2), dtype=torch.uint8)
        ops.sort_ids_stable_multi(sort, sws)
        self._segsum("lgn", [self._site_row("lgn_user", du, C, 0, C, B, dF[:Vu], None),
                             self._site_row("lgn_item", di, C, 0, C, B, dF[Vu:], None)])
        call("clsr_lgn_reg_rows", self.lg_inv, F[Vu:], dF[Vu:], Vi, C, float(hp.embed_l2), self.lg_stats, self.losses[1:], None)
        dE0, parts = prop.backward(dF, reduce=False)
        for k, part in enumerate(parts):
            self._rp(part, prop.parts, prop.part_floats, prop.part_floats, self.lg_dWb[k])
        self._dw_flush()
        # ---- dE_0 reaches the three gradient tables: user and item as they are (dense), cate as segment sums by item2cate
        tg, cs = self.tab_grad, self.lg_cate
        call("clsr_copy_cols", dE0, C, 0, 1, Vu, C, tg["user"], C, 0, 0)
        call("clsr_copy_cols", dE0[Vu:], C, 0, 1, Vi, Di, tg["item"], Di, 0, 0)
        call("clsr_lgn_rows_sum", *cs.head(), Vi, dE0[Vu:, Di:], C, Dc, tg["cate"], Dc, cs.ws)
        # (the raw cate_embedding's involved rows: the usual regulariser term, its slice's norm in slot 5)
        call("clsr_lgn_reg_rows", self.lg_inv_c, self.tables["cate"], tg["cate"], self.dims["Vc"], Dc, float(hp.embed_l2),
             self.lg_stats, self.losses[1:], ss[5:])
        call("clsr_lgn_grad_sumsq", dE0, Vu, N, C, Di, self.lg_stats, ss[6:], ss[0:], ss[1:])
        out = dict(logit=logit, dlogit=dlogit, F=F, dF=dF, dE0=dE0)
        if apply:
            self._apply_updates()
        return out

    # ------------------------------------------------------------------ NextItNet
    def _nextitnet_forward(self, f, training, early_aux=None):
        """History gather, ONE launch for the stack of blocks, the target rows into columns C .. 2C of model_output, the
        logit MLP.  Training: model_output holds Hn T G rows in (h, t, g) order (row (h, t, g) = x_L[h, t] ++ the target of
        feed row h G + g at position t) and every block's input is saved; scoring: one row per feed line, x_L[:, T - 1]."""
        B, T = f["B"], f["T"]
        D, Di, Dc, W = self.D, self.Di, self.Dc, self.out_dim
        if T != self.nx_T:
            raise ValueError("NextItNet's feed must hold max_seq_length = %d steps, got %d" % (self.nx_T, T))
        # (the reference's graph itself takes every G-th history of a training feed: nextitnet.py:29-38)
        G = self.G_train if training else ((f.get("G") or 1) if f.get("compact") else 1)
        if B % G:
            raise ValueError("feed rows (%d) must be a multiple of %d" % (B, G))
        Hn = B // G
        R = Hn * T * G if training else B
        if f["items"].numel() != R or f["cates"].numel() != R:
            raise ValueError("NextItNet %s feed: items / cates must hold %d ids per row (NextItNetIterator), got shape %r"
                             % ("training" if training else "scoring", T if training else 1, tuple(f["items"].shape)))
        self.last_shape = (R, T, G, Hn)
        self._pack_all(training)
        hs = 1 if f.get("compact") else G
        items, cates, labels = f["items"], f["cates"], f["labels"]
        if training:
            items = f["nx_items_t"] = self._buf("nx.items_t", R, dtype=torch.int32)
            cates = f["nx_cates_t"] = self._buf("nx.cates_t", R, dtype=torch.int32)
            labels = self._buf("nx.labels_t", R)
            call("clsr_nextitnet_rows", f["items"], f["cates"], f["labels"], Hn, T, G, items, cates, labels)
        step_start = self._fork_point()
        hist = self._buf("hist", Hn, T, D)
        # (the trunk's gather also writes the masked mean and the recent mean, 2 Hn D floats that nothing in this graph
        # reads: the entry point takes no NULL for them, and they are 1 / T of the launch's traffic)
        call("clsr_gather_hist_fwd", self.tables["item"], self.tables["cate"], f["item_history"],
             f["item_cate_history"], hs * T, f["seq_len"], hs, Hn, T, Di, Dc, 1, hist, self._buf("hist_mean", Hn, D),
             self._buf("hist_recent", Hn, D))
        mo = self._buf("model_output", R, W)
        tb = self.tables
        ops.multi("clsr_gather_rows_multi", ops.GatherDesc, [
            ops.GatherDesc.row(table=tb["item"], idx=items, out=mo, idx_stride=1, N=R, C=Di, ldo=W, col0=D),
            ops.GatherDesc.row(table=tb["cate"], idx=cates, out=mo, idx_stride=1, N=R, C=Dc, ldo=W, col0=D + Di)])
        if early_aux is not None or training:
            with self._branch("@aux", after=step_start):
                if early_aux is not None:
                    early_aux()
                if training:
                    self._sort_hist_ids(f, Hn, T, hs)
        saved = self._buf("nx.saved", self.nx_nb, Hn, T, D) if training else None
        call("clsr_nextitnet_fwd", hist, Hn, T, D, self.nx_W, self.nx_k, self.nx_nb, self.nx_dil, saved, mo, W, G,
             0 if training else 1)
        self._join()
        logit = self._mlp_fwd("lg", LG, mo, W, W, (self.L0, self.L1), R, training)
        return dict(hist_input=hist, model_output=mo, logit=logit, labels_t=labels, saved=saved)

    def _nextitnet_train_step(self, f, apply):
        """Marks (the 2-D items / cates included), the forward, the group softmax over G consecutive rows of every
        position, the logit MLP's backward over Hn T G rows, ONE launch back through the blocks, then the shared phases:
        the partial-sum reduction of the dense gradients, the table-gradient path, regulariser + clip + optimiser."""
        self._step = _StepState(f)
        B, T = f["B"], f["T"]
        G = self.G_train
        if B % G:
            raise ValueError("training feed rows (%d) must be a multiple of 1+train_num_ngs (%d)" % (B, G))
        Hn = B // G
        R = Hn * T * G
        D, Di, Dc, W = self.D, self.Di, self.Dc, self.out_dim
        hs = 1 if f.get("compact") else G
        zpool = self._buf("zero_pool", 2 * Hn * D)
        fl = self.tab_flags

        def zero_and_mark():
            call("clsr_zero_doubles", self.losses, 8)
            call("clsr_zero_doubles", self.sumsq_tab, 16)
            call("clsr_zero_floats", zpool, zpool.numel())
            mark = ops.MarkDesc.row
            ops.multi("clsr_mark_rows_multi", ops.MarkDesc, [
                mark(idx=f["item_history"], flags=fl["item"], nrows=Hn, row_stride=hs * T, ncols=T),
                mark(idx=f["items"], flags=fl["item"], nrows=B, row_stride=T, ncols=T),
                mark(idx=f["item_cate_history"], flags=fl["cate"], nrows=Hn, row_stride=hs * T, ncols=T),
                mark(idx=f["cates"], flags=fl["cate"], nrows=B, row_stride=T, ncols=T)])
        take = self._carver(zpool)
        # no masked mean / recent mean in this graph: the segmented sums take their gradients as arguments all the same, so
        # they get 2 Hn D zeros (zeroed with the step's other accumulators, 1 / T of d hist)
        dM, dR = take(Hn, D), take(Hn, D)
        out = self._forward(f, True, None, zero_and_mark)
        dlogit = self._buf("dlogit", R)
        call("clsr_softmax_loss", out["logit"], out["labels_t"], Hn * T, G, 1.0 / (Hn * T * self.dp_world),
             self.losses[0:], dlogit)
        dmo = self._mlp_bwd("lg", LG, dlogit, out["model_output"], W, W, W, (self.L0, self.L1), R)
        dxl, dtarget = self._buf("nx.dxl", Hn, T, D), self._buf("nx.dtarget", R, D)
        call("clsr_group_sum_cols", dmo, W, 0, G, Hn * T, D, dxl, D, 0, 0)
        call("clsr_copy_cols", dmo, W, D, 1, R, D, dtarget, D, 0, 0)
        shape = (Hn, T, D, self.nx_k, self.nx_nb)
        parts = query("clsr_nextitnet_parts", *shape)
        ws = self._buf("nx.ws", query("clsr_nextitnet_workspace_floats", *shape))
        dhist = self._buf("nx.dhist", Hn, T, D)
        # d hist (padded steps included: their rows reach table row 0) and a row of dense-gradient sums per workgroup
        call("clsr_nextitnet_bwd", dxl, out["saved"], Hn, T, D, self.nx_W, self.nx_k, self.nx_nb, self.nx_dil, dhist, ws)
        self._rp(ws, parts, self.nx_P, self.nx_P, self.nx_dW)
        self._dw_flush()
        self._join()
        # ---- embedding gradients
        ss = self.sumsq_tab
        if self.det_grads:
            # the target rows ride in the sorted lists of the history lookups: every gradient row summed in a fixed order
            self._hist_grad_sorted(dhist, dM, dR, Hn, T, f["seq_len"], hs, ss, dtarget=dtarget)
        else:
            self._hist_grad_sorted(dhist, dM, dR, Hn, T, f["seq_len"], hs, ss)
            call("clsr_scatter_add_rows", dtarget, D, 0, f["nx_items_t"], 1, R, Di, self.tab_grad["item"], ss[2:])
            call("clsr_scatter_add_rows", dtarget, D, Di, f["nx_cates_t"], 1, R, Dc, self.tab_grad["cate"], ss[3:])
        out = dict(out, dlogit=dlogit, dhist=dhist, dxl=dxl)
        if apply:
            self._apply_updates()
        return out

    def _asvd_bwd(self, dout, hist, dhist, Hn, T):
        """Backward of the A2SVD attention: d query, d attention_mat, and its two contributions to d(hist)."""
        P, Gd, D, M, sc = self.P, self.Gd, self.D, Hn * T, self.sc
        ai, w1 = self._buf("asvd.ai", M, D), self._buf("asvd.wts", Hn, T)
        dai = self._buf("asvd.dai", M, D)
        parts = query("clsr_asvd_att_bwd_parts", Hn)
        qp = self._buf("asvd.qpart", 1024 * 256)[: parts * D]
        qname = sc["asvd"] + "query"
        call("clsr_asvd_att_bwd", dout, w1, ai, P[qname], hist, Hn, T, D, dai, dhist, qp)
        self._rp(qp, parts, D, D, Gd[qname])
        self._dw(hist, D, dai, D, M, D, D, Gd[sc["asvd"] + "attention_mat"], D)
        self._gemm(dai, D, "asvd.A^T", M, D, D, dhist, D, acc=1)

    def read_losses(self):
        v = self.losses.cpu().tolist()
        return dict(data_loss=v[0], regular_loss=v[1], loss=v[0] + v[1])
