"""MultiMNIST MVAE (50x50 image of up to four digits + the digit string) on HIP -- drop-in for the reference's
``multimnist/model.py``: same constructor arguments, ``forward`` signatures, return values and ``state_dict`` keys
(``image_encoder.features.0.weight`` ... ``image_encoder.classifier.3.bias``, ``image_decoder.upsample.0.*``,
``image_decoder.hallucinate.*``, ``text_encoder.embed.weight``, ``gru.weight_ih_l0`` ... ``h2o.*``).

    MVAE             multimnist/model.py:21-72     forward / infer / reparametrize, PoE with the prior expert
    ImageEncoder     multimnist/model.py:75-111    q(z|x): four stride-2 4x4 convs 50 -> 25 -> 12 -> 6 -> 2 with
                                                   BatchNorm2d, Linear(1024, 512) + Dropout(0.1), Linear(512, 2D)
    ImageDecoder     multimnist/model.py:114-142   p(x|z): Linear(D, 1024), transposed convs 2 -> 6 -> 12 -> 25 -> 50
                                                   (the third is 5x5), logits
    TextEncoder      multimnist/model.py:145-181   q(z|y): Embedding -> bidirectional GRU -> last position,
                                                   directions summed -> Linear(200, 2D) -> (mu, logvar)
    TextDecoder      multimnist/model.py:184-235   p(y|z): 4 greedy autoregressive steps of a 2-layer GRU
    swish / Swish    multimnist/model.py:255-261
    ProductOfExperts multimnist/model.py:238-252 (the single-eps variant, as celeba's), prior_expert :264-277
    max_length, n_characters, SOS, FILL            multimnist/utils.py:12-19

The image stacks are ``Stack``s of ``layers.py``: four of their eight convolutions are geometries of the 4x4 kernel
family (csrc/conv.hip); the odd 25x25 map, the two pad-0 layers and the 5x5 transposed conv run on the general
stride-2 family (csrc/conv_gen.hip) -- ``layers.py`` picks per launch.  In the text stacks every matrix product is an
``mvae_linear_*`` launch (leading dimensions make the reference's ``torch.cat((c_in, z))`` / ``torch.cat((c_out, z))``
column ranges of one buffer), the gate arithmetic / embeddings / arg-max feedback are the K16 kernels of csrc/gru.hip;
forward and backward are hand-written (``torch.autograd.Function`` shells), no ATen arithmetic.  What the reference
evaluates but never uses is not evaluated: the backward direction of the encoder's GRU contributes only its FIRST
step (on the last character) to ``x[-1]`` (:177).  The latent path (PoE, draw, KL) is the fused ``mvae_poe_*`` launch of
the other four models.  The decoder's four greedy steps run as one launch per direction (csrc/gru_seq.hip) where
``TextDecoder.whole_sequence`` is set, the encoder as one launch per direction (csrc/gru_enc_seq.hip) where
``TextEncoder.whole_sequence`` is; the per-cell launches remain as the fallback.  There is no fused or captured
MultiMNIST step: ``train.py`` runs the modules eagerly."""
import warnings

import torch
import torch.nn as nn

from .. import kernels as K
from .. import layers as L
from ..base import MVAEBase, Stack
from ..base import ProductOfExpertsB as ProductOfExperts, prior_expert  # noqa: F401
from ..layers import Swish  # noqa: F401

max_length = 4          # multimnist/utils.py:12
all_characters = '0123456789'
n_characters = 12       # 10 digits + SOS + FILL (multimnist/utils.py:13-19)
SOS, FILL = 10, 11
KEEP = 0.9              # nn.GRU(..., dropout=0.1) between the decoder's two layers


def swish(x):
    return Swish()(x)


def _new(*shape, like):
    return torch.empty(*shape, dtype=torch.float32, device=like.device)


def _need_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError('multimodal-vae-public_amd: %s must live on the GPU (got %s); there is no CPU fallback'
                           % (what, t.device))


class GRU(nn.GRU):
    """Parameter holder with nn.GRU's names and default initialisation; the enclosing module runs the cells."""
    def forward(self, *a, **kw):
        raise RuntimeError('this GRU runs fused inside TextEncoder / TextDecoder; call the enclosing module')


def _cell_params(gru, layer, reverse=False):
    sfx = '_l%d%s' % (layer, '_reverse' if reverse else '')
    return tuple(getattr(gru, n + sfx) for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))


def _cell_fwd(x, h_prev, p, h_out):
    """One GRU cell: returns the tape entry (x, h_prev, gates)."""
    w_ih, w_hh, b_ih, b_hh = p
    B, H = h_prev.shape
    gi, gh = _new(B, 3 * H, like=x), _new(B, 3 * H, like=x)
    K.linear_fwd(x, w_ih, b_ih, gi, None)
    K.linear_fwd(h_prev, w_hh, b_hh, gh, None)
    gates = _new(B, 4 * H, like=x)
    K.gru_cell_fwd(gi, gh, h_prev, h_out, gates)
    return (x, h_prev, gates)


def _cell_bwd(dh, dh_extra, tape, p, grads, first, dx_out=None, dx_accumulate=False, want_dh_prev=True):
    """Backward of one cell.  ``grads`` = (dw_ih, dw_hh, db_ih, db_hh) (overwritten when ``first``, else added to).
    Returns (dx or None, dh_prev or None)."""
    x, h_prev, gates = tape
    w_ih, w_hh, _, _ = p
    B, H = h_prev.shape
    dgi, dgh, dh_prev = _new(B, 3 * H, like=x), _new(B, 3 * H, like=x), _new(B, H, like=x)
    K.gru_cell_bwd(dh, dh_extra, gates, h_prev, dgi, dgh, dh_prev)
    K.linear_wgrad(dgi, x, grads[0], grads[2], accumulate=not first)
    K.linear_wgrad(dgh, h_prev, grads[1], grads[3], accumulate=not first)
    dx = None
    if dx_out is not None:
        K.linear_dgrad(dgi, w_ih, dx_out, accumulate=dx_accumulate)
        dx = dx_out
    if want_dh_prev:
        K.linear_dgrad(dgh, w_hh, dh_prev, accumulate=True)
    return dx, (dh_prev if want_dh_prev else None)


# ----------------------------------------------------------------------------- encoder
class _TextEncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bidirectional, w_emb, w_h2p, b_h2p, *gru_params):
        B, L = x.shape
        H = w_emb.shape[1]
        pf = gru_params[:4]
        pr = gru_params[4:8] if bidirectional else None
        e = _new(L, B, H, like=w_emb)
        for t in range(L):
            K.embedding_fwd(x[:, t], w_emb, e[t])
        zero = torch.zeros(B, H, dtype=torch.float32, device=w_emb.device)
        tape, h_prev = [], zero
        for t in range(L):
            h = _new(B, H, like=w_emb)
            tape.append(_cell_fwd(e[t], h_prev, pf, h))
            h_prev = h
        s = _new(B, H, like=w_emb)
        K.copy2d(h_prev, s)
        tape_r = None
        if bidirectional:
            hb = _new(B, H, like=w_emb)
            tape_r = _cell_fwd(e[L - 1], zero, pr, hb)     # the backward direction's state AT the last position
            K.copy2d(hb, s, accumulate=True)
        out = _new(B, w_h2p.shape[0], like=w_emb)
        K.linear_fwd(s, w_h2p, b_h2p, out, None)
        ctx.tapes = (x, e, tape, tape_r, s)
        ctx.params = (w_emb, w_h2p, pf, pr)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, e, tape, tape_r, s = ctx.tapes
        w_emb, w_h2p, pf, pr = ctx.params
        B, L = x.shape
        H = w_emb.shape[1]
        dout = dout.contiguous()
        dw_h2p, db_h2p = torch.empty_like(w_h2p), _new(w_h2p.shape[0], like=w_emb)
        K.linear_wgrad(dout, s, dw_h2p, db_h2p)
        ds = _new(B, H, like=w_emb)
        K.linear_dgrad(dout, w_h2p, ds)
        de = _new(L, B, H, like=w_emb)
        gf = tuple(torch.empty_like(p) for p in pf)
        dh = ds
        for t in range(L - 1, -1, -1):
            _, dh = _cell_bwd(dh, None, tape[t], pf, gf, first=(t == L - 1), dx_out=de[t])
        grads_r = ()
        if pr is not None:
            gr = tuple(torch.empty_like(p) for p in pr)
            _cell_bwd(ds, None, tape_r, pr, gr, first=True, dx_out=de[L - 1], dx_accumulate=True, want_dh_prev=False)
            grads_r = gr
        dw_emb = torch.empty_like(w_emb)
        for t in range(L):
            K.embedding_bwd(x[:, t], w_emb, de[t], dw_emb, accumulate=(t > 0))
        ctx.tapes = None
        return (None, None, dw_emb, dw_h2p, db_h2p) + gf + grads_r


class _TextEncoderSeqFn(torch.autograd.Function):
    """The encoder on the whole-sequence kernels (csrc/gru_enc_seq.hip): ONE launch for the gathers, the L + 1 cells, the
    direction sum and h2p; backward: ONE launch for the reverse recurrence, then the weight gradients as Linear launches
    on the time-stacked [L * B, .] tapes and one embedding backward -- seven launches, five when unidirectional.
    ``want_tape`` is False under ``no_grad``: nothing but the output is stored then."""
    @staticmethod
    def forward(ctx, x, bidirectional, want_tape, w_emb, w_h2p, b_h2p, *gru_params):
        B, L = x.shape
        H = w_emb.shape[1]
        pf = gru_params[:4]
        pr = gru_params[4:8] if bidirectional else None
        out = _new(B, w_h2p.shape[0], like=w_emb)
        tape = None
        if want_tape:
            tape = (_new(L, B, H, like=w_emb), _new(L + 1, B, H, like=w_emb), _new(L, B, 4 * H, like=w_emb),
                    _new(B, 4 * H, like=w_emb) if bidirectional else None, _new(B, H, like=w_emb),
                    torch.empty(L, B, dtype=torch.int64, device=w_emb.device))
        K.gru_enc_seq_fwd(x, w_emb, pf, pr, w_h2p, b_h2p, out, tape)
        ctx.tapes = tape
        ctx.params = (w_emb, w_h2p, pf, pr)
        return out

    @staticmethod
    def backward(ctx, dout):
        tape = ctx.tapes
        if tape is None:
            raise RuntimeError('TextEncoder: backward through a forward that ran without gradient tracking')
        e_all, h_all, gates, gates_r, s, idx_all = tape
        w_emb, w_h2p, pf, pr = ctx.params
        L, B, H = e_all.shape
        dout = dout.contiguous()
        dgi, dgh, de = _new(L, B, 3 * H, like=w_emb), _new(L, B, 3 * H, like=w_emb), _new(L, B, H, like=w_emb)
        dgi_r = dgh_r = None
        if pr is not None:
            dgi_r, dgh_r = _new(B, 3 * H, like=w_emb), _new(B, 3 * H, like=w_emb)
        K.gru_enc_seq_bwd(dout, w_h2p, pf, pr, w_emb.shape[0], h_all, gates, gates_r, dgi, dgh, dgi_r, dgh_r, de)
        dw_h2p, db_h2p = torch.empty_like(w_h2p), _new(w_h2p.shape[0], like=w_emb)
        K.linear_wgrad(dout, s, dw_h2p, db_h2p)
        R = L * B
        gf = tuple(torch.empty_like(p) for p in pf)
        K.linear_wgrad(dgi.view(R, 3 * H), e_all.view(R, H), gf[0], gf[2])
        K.linear_wgrad(dgh.view(R, 3 * H), h_all[:L].view(R, H), gf[1], gf[3])        # h_prev of position t = slot t
        grads_r = ()
        if pr is not None:
            grads_r = tuple(torch.empty_like(p) for p in pr)
            K.linear_wgrad(dgi_r, e_all[L - 1], grads_r[0], grads_r[2])
            K.linear_wgrad(dgh_r, h_all[0], grads_r[1], grads_r[3])                   # h_prev = 0: weight_hh's is zero
        dw_emb = torch.empty_like(w_emb)
        K.embedding_bwd(idx_all.view(R), w_emb, de.view(R, H), dw_emb)
        ctx.tapes = None
        return (None, None, None, dw_emb, dw_h2p, db_h2p) + gf + grads_r


class TextEncoder(nn.Module):
    """Parametrizes q(z|y) (multimnist/model.py:145-179).  ``whole_sequence`` (an attribute, not a constructor argument)
    selects the one-launch kernels of csrc/gru_enc_seq.hip where ``kernels.gru_enc_seq_supported`` takes the geometry;
    False runs the per-cell launches."""
    WHOLE_SEQUENCE_DEFAULT = True       # profiles/multimnist_gru_enc_seq.txt

    def __init__(self, n_latents, n_characters, n_hiddens=200, bidirectional=True):
        super().__init__()
        self.embed = nn.Embedding(n_characters, n_hiddens)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')     # "dropout expects num_layers > 1": the reference asks for the same GRU
            self.gru = GRU(n_hiddens, n_hiddens, 1, dropout=0.1, bidirectional=bidirectional)
        self.h2p = nn.Linear(n_hiddens, n_latents * 2)
        self.n_latents = n_latents
        self.n_hiddens = n_hiddens
        self.bidirectional = bidirectional
        self.whole_sequence = self.WHOLE_SEQUENCE_DEFAULT

    def heads(self, x):
        """The [batch, 2D] output of ``h2p`` (mu | logvar), as the fused PoE launch takes it."""
        _need_gpu(x, 'text'); _need_gpu(self.embed.weight, 'the module')
        if x.dim() != 2 or x.dtype != torch.int64:
            raise ValueError('text must be an int64 [batch, length] tensor of character indices')
        params = _cell_params(self.gru, 0) + (_cell_params(self.gru, 0, True) if self.bidirectional else ())
        if self.whole_sequence and K.gru_enc_seq_supported(x.shape[0], self.n_hiddens, 2 * self.n_latents,
                                                           self.embed.weight.shape[0], x.shape[1], self.bidirectional):
            all_params = (self.embed.weight, self.h2p.weight, self.h2p.bias) + params
            want_tape = torch.is_grad_enabled() and any(p.requires_grad for p in all_params)
            return _TextEncoderSeqFn.apply(x.contiguous(), self.bidirectional, want_tape, *all_params)
        return _TextEncoderFn.apply(x.contiguous(), self.bidirectional, self.embed.weight, self.h2p.weight, self.h2p.bias,
                                    *params)

    def forward(self, x):
        p = self.heads(x)
        return p[:, :self.n_latents], p[:, self.n_latents:]


# ----------------------------------------------------------------------------- decoder
class _TextDecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, masks, holder, w_emb, w_z2h, b_z2h, w_h2o, b_h2o, *gru_params):
        z = z.contiguous()
        B, D = z.shape
        H = w_emb.shape[1]
        p0, p1 = gru_params[:4], gru_params[4:8]
        n_chars = w_h2o.shape[0]
        dev = z.device
        hz = _new(B, H, like=z)
        K.linear_fwd(z, w_z2h, b_z2h, hz, None)
        h0_prev = h1_prev = hz
        c_in = torch.full((B,), SOS, dtype=torch.int64, device=dev)
        words = _new(B, max_length, n_chars, like=z)
        steps = []
        for i in range(max_length):
            xcat = _new(B, H + D, like=z)
            K.embedding_fwd(c_in, w_emb, xcat[:, :H], swish=True)          # swish(self.embed(c_in))  (:220)
            K.copy2d(z, xcat[:, H:])                                       # torch.cat((c_in, z), dim=1) (:221)
            h0 = _new(B, H, like=z)
            t0 = _cell_fwd(xcat, h0_prev, p0, h0)
            if masks is not None:                                          # nn.GRU's Dropout between its two layers
                d0 = _new(B, H, like=z)
                K.copy2d(h0, d0, mask=masks[i], scale=1.0 / KEEP)
            else:
                d0 = h0
            ocat = _new(B, H + D, like=z)
            t1 = _cell_fwd(d0, h1_prev, p1, ocat[:, :H])                   # c_out lands in the cat buffer (:224-225)
            K.copy2d(z, ocat[:, H:])
            K.linear_fwd(ocat, w_h2o, b_h2o, words[:, i, :], None)         # words[:, i] = self.h2o(...) (:212,226)
            steps.append((c_in, t0, t1, ocat))
            nxt = torch.empty(B, dtype=torch.int64, device=dev)
            K.argmax_rows(words[:, i, :], nxt)                             # greedy feedback (:211,213)
            c_in = nxt
            h0_prev, h1_prev = h0, ocat[:, :H]
        holder['fed'] = torch.stack([s[0] for s in steps])
        ctx.tapes = (z, masks, hz, steps)
        ctx.params = (w_emb, w_z2h, w_h2o, p0, p1)
        return words

    @staticmethod
    def backward(ctx, dwords):
        z, masks, hz, steps = ctx.tapes
        w_emb, w_z2h, w_h2o, p0, p1 = ctx.params
        B, D = z.shape
        H = w_emb.shape[1]
        dwords = dwords.contiguous()
        dz = torch.zeros_like(z)
        dw_h2o, db_h2o = torch.empty_like(w_h2o), _new(w_h2o.shape[0], like=z)
        g0 = tuple(torch.empty_like(p) for p in p0)
        g1 = tuple(torch.empty_like(p) for p in p1)
        dw_emb = torch.empty_like(w_emb)
        dh0_carry = torch.zeros(B, H, dtype=torch.float32, device=z.device)
        dh1_carry = torch.zeros(B, H, dtype=torch.float32, device=z.device)
        for i in range(max_length - 1, -1, -1):
            c_in, t0, t1, ocat = steps[i]
            first = i == max_length - 1
            dlog = dwords[:, i, :]
            K.linear_wgrad(dlog, ocat, dw_h2o, db_h2o, accumulate=not first)
            d_ocat = _new(B, H + D, like=z)
            K.linear_dgrad(dlog, w_h2o, d_ocat)
            K.copy2d(d_ocat[:, H:], dz, accumulate=True)
            dd0 = _new(B, H, like=z)
            _, dh1_carry = _cell_bwd(d_ocat[:, :H], dh1_carry, t1, p1, g1, first, dx_out=dd0)
            if masks is not None:
                dd0m = _new(B, H, like=z)
                K.copy2d(dd0, dd0m, mask=masks[i], scale=1.0 / KEEP)
                dd0 = dd0m
            dxcat = _new(B, H + D, like=z)
            _, dh0_carry = _cell_bwd(dd0, dh0_carry, t0, p0, g0, first, dx_out=dxcat)
            K.copy2d(dxcat[:, H:], dz, accumulate=True)
            K.embedding_bwd(c_in, w_emb, dxcat[:, :H], dw_emb, swish=True, accumulate=not first)
        dhz = _new(B, H, like=z)
        K.copy2d(dh0_carry, dhz)
        K.copy2d(dh1_carry, dhz, accumulate=True)          # z2h(z) initialises BOTH layers (.repeat(2, 1, 1), :207)
        dw_z2h, db_z2h = torch.empty_like(w_z2h), _new(w_z2h.shape[0], like=z)
        K.linear_wgrad(dhz, z, dw_z2h, db_z2h)
        K.linear_dgrad(dhz, w_z2h, dz, accumulate=True)
        ctx.tapes = None
        return (dz, None, None, dw_emb, dw_z2h, db_z2h, dw_h2o, db_h2o) + g0 + g1


class _TextDecoderSeqFn(torch.autograd.Function):
    """The decoder on the whole-sequence kernels (csrc/gru_seq.hip): z2h, ONE launch for the four greedy steps of both GRU
    layers + h2o + arg-max; backward: ONE launch for the reverse recurrence, then the weight gradients as five launches
    on the time-stacked [L * B, .] tapes.  ``masks`` is one [L, B, H] tensor (or None), ``want_tape`` False under
    ``no_grad``: nothing but the logits and the fed characters is stored then."""
    @staticmethod
    def forward(ctx, z, masks, holder, want_tape, w_emb, w_z2h, b_z2h, w_h2o, b_h2o, *gru_params):
        z = z.contiguous()
        B, D = z.shape
        H = w_emb.shape[1]
        p0, p1 = gru_params[:4], gru_params[4:8]
        n_chars, L = w_h2o.shape[0], max_length
        hz = _new(B, H, like=z)
        K.linear_fwd(z, w_z2h, b_z2h, hz, None)
        words = _new(B, L, n_chars, like=z)
        fed = torch.empty(L, B, dtype=torch.int64, device=z.device)
        tape = None
        if want_tape:
            tape = (_new(L, B, H + D, like=z), _new(L + 1, B, H, like=z), _new(L + 1, B, H, like=z), _new(L, B, H, like=z),
                    _new(L, B, H + D, like=z), _new(L, B, 4 * H, like=z), _new(L, B, 4 * H, like=z))
        K.gru_dec_seq_fwd(z, hz, w_emb, p0, p1, w_h2o, b_h2o, masks, 1.0 / KEEP, words, tape, fed, SOS)
        holder['fed'] = fed
        ctx.tapes = (z, masks, fed, tape)
        ctx.params = (w_emb, w_z2h, w_h2o, p0, p1)
        return words

    @staticmethod
    def backward(ctx, dwords):
        z, masks, fed, tape = ctx.tapes
        if tape is None:
            raise RuntimeError('TextDecoder: backward through a forward that ran without gradient tracking')
        xcat_all, h0_all, h1_all, d0_all, ocat_all, gates0, gates1 = tape
        w_emb, w_z2h, w_h2o, p0, p1 = ctx.params
        B, D = z.shape
        H = w_emb.shape[1]
        n_chars, L = w_h2o.shape[0], max_length
        dwords = dwords.contiguous()
        dgi0, dgh0, dgi1, dgh1 = (_new(L, B, 3 * H, like=z) for _ in range(4))
        demb, dlog = _new(L, B, H, like=z), _new(L, B, n_chars, like=z)
        dhz, dz = _new(B, H, like=z), _new(B, D, like=z)
        K.gru_dec_seq_bwd(dwords, p0, p1, w_h2o, masks, 1.0 / KEEP, h0_all, h1_all, gates0, gates1, dgi0, dgh0, dgi1, dgh1,
                          demb, dlog, dhz, dz)
        g0 = tuple(torch.empty_like(p) for p in p0)
        g1 = tuple(torch.empty_like(p) for p in p1)
        R = L * B
        K.linear_wgrad(dgi0.view(R, 3 * H), xcat_all.view(R, H + D), g0[0], g0[2])
        K.linear_wgrad(dgh0.view(R, 3 * H), h0_all[:L].view(R, H), g0[1], g0[3])       # h_prev of step i = slot i
        K.linear_wgrad(dgi1.view(R, 3 * H), d0_all.view(R, H), g1[0], g1[2])
        K.linear_wgrad(dgh1.view(R, 3 * H), h1_all[:L].view(R, H), g1[1], g1[3])
        dw_h2o, db_h2o = torch.empty_like(w_h2o), _new(n_chars, like=z)
        K.linear_wgrad(dlog.view(R, n_chars), ocat_all.view(R, H + D), dw_h2o, db_h2o)
        dw_emb = torch.empty_like(w_emb)
        K.embedding_bwd(fed.view(R), w_emb, demb.view(R, H), dw_emb, swish=True)
        dw_z2h, db_z2h = torch.empty_like(w_z2h), _new(w_z2h.shape[0], like=z)
        K.linear_wgrad(dhz, z, dw_z2h, db_z2h)
        K.linear_dgrad(dhz, w_z2h, dz, accumulate=True)
        ctx.tapes = None
        return (dz, None, None, None, dw_emb, dw_z2h, db_z2h, dw_h2o, db_h2o) + g0 + g1


class TextDecoder(nn.Module):
    """Parametrizes p(y|z) (multimnist/model.py:182-228).  ``forward(z)`` returns the [batch, 4, n_characters] logits;
    ``dropout_masks`` (4 tensors [batch, 200] in {0, 1}) replays a host draw in parity runs, otherwise the training-mode
    masks come from the device Philox stream.  ``last_fed`` holds the characters fed back ([4, batch]).
    ``whole_sequence`` (an attribute, not a constructor argument) selects the one-launch kernels of csrc/gru_seq.hip
    where ``kernels.gru_dec_seq_supported`` takes the geometry; False runs the per-cell launches."""
    WHOLE_SEQUENCE_DEFAULT = True       # profiles/multimnist_gru_seq.txt

    def __init__(self, n_latents, n_characters, n_hiddens=200):
        super().__init__()
        self.embed = nn.Embedding(n_characters, n_hiddens)
        self.z2h = nn.Linear(n_latents, n_hiddens)
        self.gru = GRU(n_hiddens + n_latents, n_hiddens, 2, dropout=0.1)
        self.h2o = nn.Linear(n_hiddens + n_latents, n_characters)
        self.n_latents = n_latents
        self.n_characters = n_characters
        self.n_hiddens = n_hiddens
        self.last_fed = None
        self.whole_sequence = self.WHOLE_SEQUENCE_DEFAULT
        self.__dict__['_rng'] = None

    def seed_noise(self, seed):
        self.__dict__['_rng'] = (int(seed), torch.zeros(1, dtype=torch.int64, device=self.embed.weight.device))

    def _device_mask_tensor(self, B):
        st = self.__dict__.get('_rng')
        if st is None or st[1].device != self.embed.weight.device:
            self.seed_noise(0x5DEECE66D)
            st = self.__dict__['_rng']
        masks = torch.empty(max_length, B, self.n_hiddens, dtype=torch.float32, device=self.embed.weight.device)
        K.bernoulli_(masks, KEEP, st[0], st[1])
        return masks

    def _device_masks(self, B):
        masks = self._device_mask_tensor(B)
        return [masks[i] for i in range(max_length)]

    def forward(self, z, dropout_masks=None):
        _need_gpu(z, 'z'); _need_gpu(self.embed.weight, 'the module')
        masks = None
        seq = self.whole_sequence and K.gru_dec_seq_supported(z.shape[0], self.n_hiddens, self.n_latents,
                                                              self.n_characters, max_length)
        if self.training:
            if dropout_masks is None:
                masks = self._device_mask_tensor(z.shape[0]) if seq else self._device_masks(z.shape[0])
            else:
                masks = [m.to(z.device).float().contiguous() for m in dropout_masks]
                if len(masks) != max_length or any(m.shape != (z.shape[0], self.n_hiddens) for m in masks):
                    raise ValueError('dropout_masks: %d tensors of [batch, %d]' % (max_length, self.n_hiddens))
        holder = {}
        params = (self.embed.weight, self.z2h.weight, self.z2h.bias, self.h2o.weight, self.h2o.bias) + \
            _cell_params(self.gru, 0) + _cell_params(self.gru, 1)
        if seq:
            if isinstance(masks, list):
                masks = torch.stack(masks)
            want_tape = torch.is_grad_enabled() and (z.requires_grad or any(p.requires_grad for p in params))
            words = _TextDecoderSeqFn.apply(z.float(), masks, holder, want_tape, *params)
            self.last_fed = holder.get('fed')
            return words
        words = _TextDecoderFn.apply(z.float(), masks, holder, self.embed.weight, self.z2h.weight, self.z2h.bias,
                                     self.h2o.weight, self.h2o.bias, *(_cell_params(self.gru, 0) + _cell_params(self.gru, 1)))
        self.last_fed = holder.get('fed')
        return words


# ----------------------------------------------------------------------------- image stacks
class ImageEncoder(Stack):
    """Parametrizes q(z|x) (multimnist/model.py:75-111).  ``dropout_mask`` ([batch, 512] in {0, 1}) replays a host draw of
    the classifier's Dropout(0.1) in parity runs; otherwise the training-mode mask comes from the device Philox stream."""
    def __init__(self, n_latents):
        super().__init__()
        self.features = nn.Sequential(
            L.Conv2d(1, 32, 4, 2, 1, bias=False), L.Swish(),
            L.Conv2d(32, 64, 4, 2, 1, bias=False), L.BatchNorm2d(64), L.Swish(),
            L.Conv2d(64, 128, 4, 2, 1, bias=False), L.BatchNorm2d(128), L.Swish(),
            L.Conv2d(128, 256, 4, 2, 0, bias=False), L.BatchNorm2d(256), L.Swish())
        self.classifier = nn.Sequential(
            L.Linear(256 * 2 * 2, 512), L.Swish(), L.Dropout(p=0.1), L.Linear(512, n_latents * 2))
        self.n_latents = n_latents

    def stack_modules(self):
        return [self.features, L.View(256 * 2 * 2), self.classifier]

    def heads(self, x, dropout_mask=None):
        masks = None
        if self.training:
            if dropout_mask is None:
                owner = self.__dict__.get('_owner')
                if owner is None:
                    raise RuntimeError('encoder is not attached to an MVAE (needed for device-side dropout noise); '
                                       'pass dropout_mask explicitly')
                dropout_mask = owner.device_bernoulli(0.9, x.shape[0], 512)
            masks = [dropout_mask.contiguous().float()]
        return self.run(x, masks=masks)

    def forward(self, x, dropout_mask=None):
        h = self.heads(x, dropout_mask)
        return h[:, :self.n_latents], h[:, self.n_latents:]


class ImageDecoder(Stack):
    """Parametrizes p(x|z) (multimnist/model.py:114-142): [batch, 1, 50, 50] logits."""
    def __init__(self, n_latents):
        super().__init__()
        self.upsample = nn.Sequential(L.Linear(n_latents, 256 * 2 * 2), L.Swish())
        self.hallucinate = nn.Sequential(
            L.ConvTranspose2d(256, 128, 4, 2, 0, bias=False), L.BatchNorm2d(128), L.Swish(),
            L.ConvTranspose2d(128, 64, 4, 2, 1, bias=False), L.BatchNorm2d(64), L.Swish(),
            L.ConvTranspose2d(64, 32, 5, 2, 1, bias=False), L.BatchNorm2d(32), L.Swish(),
            L.ConvTranspose2d(32, 1, 4, 2, 1, bias=False))

    def stack_modules(self):
        return [self.upsample, L.View(256, 2, 2), self.hallucinate]

    def forward(self, z):
        return self.run(z)  # NOTE: logits, no sigmoid


# ----------------------------------------------------------------------------- the model
class MVAE(MVAEBase):
    """multimnist/model.py:21-72.  ``forward(image=None, text=None)`` -> (img_recon, txt_recon, mu, logvar); the
    keyword-only ``eps`` ([batch, D]), ``dropout_mask`` ([batch, 512]) and ``text_dropout_masks`` (4 x [batch, 200])
    replay host draws in parity runs -- without them the noise comes from the device Philox streams."""
    POE_VARIANT = 'B'
    KIND = 'multimnist'
    LABEL_KIND = 'text'
    HAS_BN = True
    IMAGE_SHAPE = (1, 50, 50)

    def __init__(self, n_latents):
        super().__init__(n_latents)
        self.image_encoder = ImageEncoder(n_latents)
        self.image_decoder = ImageDecoder(n_latents)
        self.text_encoder = TextEncoder(n_latents, n_characters, n_hiddens=200, bidirectional=True)
        self.text_decoder = TextDecoder(n_latents, n_characters, n_hiddens=200)
        self.image_encoder.__dict__['_owner'] = self

    def arena_order(self):
        return [self.image_decoder, self.text_decoder, self.text_encoder, self.image_encoder]

    def text_grad_range(self):
        """Arena range of the text stacks' parameters.  Their gradients arrive through autograd (the image stacks'
        kernels write theirs into the arena themselves): ``attach_text_grads`` points those parameters' ``.grad`` at
        the gradient arena, cleared, so that the arena-wide Adam launch finds every gradient in place."""
        ranges = self.finalize().module_ranges
        (a0, a1), (b0, b1) = ranges[self.text_decoder], ranges[self.text_encoder]
        return min(a0, b0), max(a1, b1)

    def attach_text_grads(self):
        arena = self.finalize()
        lo, hi = self.text_grad_range()
        K.fill_(arena.grad[lo:hi], 0.0)
        for mod in (self.text_decoder, self.text_encoder):
            for p in mod.parameters():
                p.grad = arena.grad_view(p)

    def forward(self, image=None, text=None, *, eps=None, dropout_mask=None, text_dropout_masks=None):
        mu, logvar, z = self._infer(image, text, eps, dropout_mask, want_z=True)
        self.__dict__['last_z'] = z.detach()        # the reference does not return the draw; parity runs read it here
        return self.image_decoder(z), self.text_decoder(z, dropout_masks=text_dropout_masks), mu, logvar

    def infer(self, image=None, text=None):
        mu, logvar, _ = self._infer(image, text, None, None, want_z=False)
        return mu, logvar

    def _infer(self, image, text, eps, dropout_mask, want_z):
        self.finalize()
        heads = []
        if image is not None:
            heads.append(self.image_encoder.heads(image, dropout_mask))
        if text is not None:
            heads.append(self.text_encoder.heads(text))
        if not heads:
            raise ValueError('at least one modality is required')
        return self._fuse(heads, eps, want_z)
