"""Conditional generation from the CelebA-19 MVAE (an image and 18 separate attribute experts): the ``sample.py`` the
reference's README promises per experiment folder and never published for ``celeba19``.  Each attribute is its own
expert, so "this face, with Eyeglasses=1 and Smiling=0" is the product of exactly the experts named -- and a batch of
CONDITION ROWS that each name their own subset (a sweep over every attribute value, imputing the missing attributes of a
data set) is one launch here:

    table  = expert_table(model)        [18, 2, 2D]: in eval mode an AttributeEncoder reads its {0, 1} input through
                                        Embedding(2, 512), so it has two possible heads; the 36 heads of a model are
                                        computed once, as grouped launches on the parameter arena
    heads  = image encoder              [rows, 2D], once per conditioning image
    mu, logvar, z = kernels.poe_table_draw(table, state, ..., img_heads, img_row, ...)        (K27, csrc/poe_table.hip)
                                        state [C, 18] in {-1 absent, 0, 1} picks a table row per attribute, img_row [C]
                                        an image row or -1; PoE variant B with the prior built in, n draws per row
    image  = sigmoid(image_decoder(z))  [n, C, 3, 64, 64]
    attrs  = sigmoid(attribute decoders(z))  [n, C, 18]: ``loglike.AttrExperts`` layers 1 - 3, the grouped N = 1 Linear
                                        and ``sigmoid_fwd`` -- the kernels that were there

``MVAE.infer`` takes None per modality for the whole batch, as the reference does: the same sweep costs one ``infer``
call per row there, about twenty launches each (tools/celeba19_sample_bench.py times both; only this path ships).

Measured on an MI355X (tools/celeba19_sample_bench.py, profiles/celeba19_sample.txt): see the README's "CelebA-19
sampling" paragraph."""
import os
import sys

if __package__ in (None, ''):      # executed as a script (`python celeba19/sample.py`)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.celeba19'

import torch  # noqa: E402

from .. import kernels as K  # noqa: E402
from .. import layers as L  # noqa: E402
from ..draws import eval_mode  # noqa: E402
from .loglike import ATTRIBUTES, AttrExperts  # noqa: E402
from .model import N_ATTRS  # noqa: E402

IMAGE_SHAPE = (3, 64, 64)
DECODE_ROWS = 4096                   # rows per decoder pass (the activations of 18 experts x 512 are held twice)
_NAMES = ', '.join('%d %s' % (i, n) for i, n in enumerate(ATTRIBUTES))


# ----------------------------------------------------------------------------- conditions (host)
def parse_conditions(spec):
    """``"Male=1,Eyeglasses=0"`` -> a state row: a list of 18 values, -1 where the attribute is not named.  An attribute
    is a name of ``ATTRIBUTES`` or its index 0 .. 17; a bare name means ``=1``; an empty spec is the prior row."""
    row = [-1] * N_ATTRS
    for item in (s.strip() for s in str(spec or '').split(',')):
        if not item:
            continue
        name, _, value = item.partition('=')
        name, value = name.strip(), value.strip() if '=' in item else '1'
        if name in ATTRIBUTES:
            a = ATTRIBUTES.index(name)
        elif name.isdigit() and int(name) < N_ATTRS:
            a = int(name)
        else:
            raise ValueError('unknown attribute %r in %r; the 18 attributes are: %s' % (name, spec, _NAMES))
        if value not in ('0', '1'):
            raise ValueError('attribute %s: the value must be 0 or 1, got %r in %r; the 18 attributes are: %s'
                             % (ATTRIBUTES[a], value, spec, _NAMES))
        if row[a] != -1:
            raise ValueError('attribute %s is named twice in %r; the 18 attributes are: %s' % (ATTRIBUTES[a], spec, _NAMES))
        row[a] = int(value)
    return row


def sweep_states():
    """The 37 rows of the sweep as an int8 [37, 18] tensor: the prior (nothing present), then (attribute a, value v) for
    a = 0 .. 17 and v = 0, 1 -- one attribute present per row."""
    state = torch.full((1 + 2 * N_ATTRS, N_ATTRS), -1, dtype=torch.int8)
    for a in range(N_ATTRS):
        for v in (0, 1):
            state[1 + 2 * a + v, a] = v
    return state


def sweep_labels():
    return ['prior'] + ['%s=%d' % (ATTRIBUTES[a], v) for a in range(N_ATTRS) for v in (0, 1)]


def tensor_to_attributes(tensor):
    """18 probabilities -> names of the attributes above 0.5 (celeba/datasets.py:138-152)."""
    return [ATTRIBUTES[i] for i in range(tensor.size(0)) if torch.round(tensor[i]) > 0.5]


# ----------------------------------------------------------------------------- the expert table
def expert_table(model):
    """[18, 2, 2D]: row (a, v) is attribute encoder a's head (mu, then logvar) for the input value v.  Three grouped
    launches on the arena for all 36 heads: Embedding + Swish, Linear + Swish, Linear.  Eval mode, no gradients."""
    model.finalize()
    gp = L.GroupedPlans([enc.plan() for enc in model.attr_encoders])
    plan = gp.plans[0]
    if [(op.kind, bool(op.act)) for op in plan] != [('emb', True), ('lin', True), ('lin', False)]:
        raise RuntimeError('celeba19 sample: the attribute encoders are not Embedding + Swish, Linear + Swish, Linear')
    dev = next(model.parameters()).device
    G = gp.G
    with eval_mode(model.attr_encoders):
        values = torch.tensor([[0.0] * G, [1.0] * G], dtype=torch.float32, device=dev)       # [2 rows, G]
        w0, w_gs, _, _ = gp.layer(0)
        if w0.shape[0] != 2:
            raise RuntimeError('celeba19 sample: the attribute encoders must start with Embedding(2, .)')
        h = torch.empty(G, 2, w0.shape[1], dtype=torch.float32, device=dev)
        K.embedding_swish_fwd_grouped(values, w0, w_gs, h)
        w0, w_gs, b0, b_gs = gp.layer(1)
        a = torch.empty(G, 2, w0.shape[0], dtype=torch.float32, device=dev)
        K.linear_fwd_grouped(h, w0, w_gs, b0, b_gs, None, a)
        w0, w_gs, b0, b_gs = gp.layer(2)
        table = torch.empty(G, 2, w0.shape[0], dtype=torch.float32, device=dev)
        K.linear_fwd_grouped(a, w0, w_gs, b0, b_gs, table, None)
    if table.shape[2] != 2 * model.n_latents:
        raise RuntimeError('celeba19 sample: the attribute encoders must end in Linear(., 2 * n_latents)')
    return table


# ----------------------------------------------------------------------------- generate
def _check(model, image, img_row, state, n_samples, eps):
    """Every refusal, before anything is launched.  Returns (state int8 [C, 18], img_row int32 [C] or None) on the host."""
    if getattr(model, 'KIND', None) != 'celeba19':
        raise ValueError('celeba19 generate: expected the celeba19 MVAE, got %r' % type(model).__name__)
    if image is not None and (not torch.is_tensor(image) or image.dim() != 4 or tuple(image.shape[1:]) != IMAGE_SHAPE
                              or image.shape[0] < 1):
        raise ValueError('celeba19 generate: `image` must be [rows >= 1, 3, 64, 64], got %s'
                         % (tuple(image.shape) if torch.is_tensor(image) else type(image).__name__,))
    rows = image.shape[0] if image is not None else 0
    if state is not None:
        state = torch.as_tensor(state)
        if state.is_cuda:
            state = state.cpu()
        if state.dim() != 2 or state.shape[1] != N_ATTRS or state.shape[0] < 1:
            raise ValueError('celeba19 generate: `state` must be [C >= 1, %d], got %s' % (N_ATTRS, tuple(state.shape)))
        if state.dtype.is_floating_point:
            if not bool((state == state.round()).all()):
                raise ValueError('celeba19 generate: `state` holds a value outside {-1 (absent), 0, 1}')
            state = state.to(torch.int64)
        if state.dtype == torch.bool or bool(((state < -1) | (state > 1)).any()):
            raise ValueError('celeba19 generate: `state` holds a value outside {-1 (absent), 0, 1}')
    if img_row is not None:
        img_row = torch.as_tensor(img_row)
        if img_row.is_cuda:
            img_row = img_row.cpu()
        if img_row.dim() != 1 or img_row.dtype.is_floating_point or img_row.dtype == torch.bool:
            raise ValueError('celeba19 generate: `img_row` must be an integer vector [C], got %s %s'
                             % (img_row.dtype, tuple(img_row.shape)))
    C = state.shape[0] if state is not None else (img_row.shape[0] if img_row is not None else max(rows, 1))
    if C < 1:
        raise ValueError('celeba19 generate: no condition rows')
    if state is None:
        state = torch.full((C, N_ATTRS), -1, dtype=torch.int8)
    if img_row is None and image is not None:
        if rows != C:
            raise ValueError('celeba19 generate: %d images for %d condition rows: pass `img_row` [C] to say which image '
                             'each row uses (-1 for none)' % (rows, C))
        img_row = torch.arange(C)
    if img_row is not None:
        if img_row.shape[0] != C:
            raise ValueError('celeba19 generate: `img_row` holds %d entries for %d condition rows' % (img_row.shape[0], C))
        if image is None and bool((img_row >= 0).any()):
            raise ValueError('celeba19 generate: `img_row` names an image row but no `image` was passed')
        if bool(((img_row < -1) | (img_row >= max(rows, 1))).any()) and image is not None:
            raise ValueError('celeba19 generate: `img_row` must lie in [-1, %d)' % rows)
        if image is None:
            img_row = None
    n = int(n_samples)
    if n < 0:
        raise ValueError('celeba19 generate: n_samples must be at least 0 (0 decodes the mean), got %r' % (n_samples,))
    if eps is not None and (n < 1 or tuple(eps.shape) != (n, C, model.n_latents)):
        raise ValueError('celeba19 generate: eps must be [n_samples, C, D] = %s with n_samples >= 1, got %s'
                         % ((n, C, model.n_latents), tuple(eps.shape)))
    if not next(model.parameters()).is_cuda:
        raise RuntimeError('celeba19 generate: the model must live on the GPU (model.cuda()); the HIP path has no CPU '
                           'fallback')
    return state.to(torch.int8).contiguous(), (img_row.to(torch.int32).contiguous() if img_row is not None else None)


def decode(model, zr):
    """zr [R, D] -> (image probabilities [R, 3, 64, 64], attribute probabilities [R, 18]), in passes of ``DECODE_ROWS``."""
    R = zr.shape[0]
    dev = zr.device
    image = torch.empty((R,) + IMAGE_SHAPE, dtype=torch.float32, device=dev)
    attrs = torch.empty(R, N_ATTRS, dtype=torch.float32, device=dev)
    rows = min(R, DECODE_ROWS)
    experts = AttrExperts(model, 0, N_ATTRS - 1, rows, dev)
    w0, w_gs, b0, b_gs = experts.layers[3]
    logits = torch.empty(N_ATTRS, rows, 1, dtype=torch.float32, device=dev)
    probs = torch.empty_like(logits)
    for r0 in range(0, R, rows):
        zc = zr[r0:r0 + rows]
        r = zc.shape[0]
        img_logits = model.image_decoder(zc).reshape(r, -1).contiguous()
        K.sigmoid_fwd(img_logits, image[r0:r0 + r].view(r, -1))
        h = experts.hidden(zc)
        lg, pr = logits.view(-1)[:N_ATTRS * r].view(N_ATTRS, r, 1), probs.view(-1)[:N_ATTRS * r].view(N_ATTRS, r, 1)
        K.linear_fwd_grouped(h, w0, w_gs, b0, b_gs, lg, None)
        K.sigmoid_fwd(lg, pr)
        attrs[r0:r0 + r] = pr.view(N_ATTRS, r).t()                       # [18, r] -> [r, 18]
    return image, attrs


def generate(model, image=None, img_row=None, state=None, n_samples=64, eps=None, seed=0):
    """Samples from the posteriors of C condition rows.  ``state`` [C, 18] with -1 (attribute absent) / 0 / 1 (default:
    nothing present); ``image`` [rows, 3, 64, 64], run once through the image encoder, with ``img_row`` [C] naming the
    image row of each condition or -1 (default: row c for condition c, which needs rows == C).  Without both there is one
    row, the prior.

    Returns a dict: ``mu``, ``logvar`` [C, D]; ``z`` [n, C, D]; ``image`` [n, C, 3, 64, 64] and ``attrs`` [n, C, 18]
    probabilities.  ``n_samples=0`` decodes the mean (z = mu, eval-mode ``reparametrize``) and the leading dimension is 1.
    ``eps`` [n, C, D] replaces the device draw (parity runs); otherwise the noise is the device Philox stream of ``seed``.
    The model is put in ``eval()`` for the call and every module's mode is restored afterwards."""
    state, img_row = _check(model, image, img_row, state, n_samples, eps)
    n, C, D = int(n_samples), state.shape[0], model.n_latents
    dev = next(model.parameters()).device
    with eval_mode(model):
        table = expert_table(model)
        heads = None
        if img_row is not None:
            heads = model.image_encoder.heads(image.to(dev).float().contiguous())
        mu = torch.empty(C, D, dtype=torch.float32, device=dev)
        logvar = torch.empty_like(mu)
        z = torch.empty(n, C, D, dtype=torch.float32, device=dev) if n else None
        if n and eps is not None:
            K.poe_table_draw(table, state, mu, logvar, z, img_heads=heads, img_row=img_row,
                             eps=eps.to(dev).float().contiguous())
        else:
            counter = torch.zeros(1, dtype=torch.int64, device=dev) if n else None
            K.poe_table_draw(table, state, mu, logvar, z, img_heads=heads, img_row=img_row,
                             seed=int(seed) & 0xFFFFFFFFFFFFFFFF, counter_dev=counter)
        if z is None:
            z = mu.view(1, C, D)
        probs_image, probs_attrs = decode(model, z.reshape(-1, D))
    lead =z.shape[0]
    return {'mu': mu, 'logvar': logvar, 'z': z, 'image': probs_image.view((lead, C) + IMAGE_SHAPE),
            'attrs': probs_attrs.view(lead, C, N_ATTRS)}


# ----------------------------------------------------------------------------- the sample.py drop-in
_transform = None


def load_condition_image(path, device='cuda'):
    """``--image-file``: a .npy / .pt array in [0, 1] (``sample_common.load_image``), or an image file decoded with Pillow
    and passed through the Resize(64) + CenterCrop(64) + ToTensor launch -> [1, 3, 64, 64] on the device."""
    from ..sample_common import load_image
    if path.endswith('.npy') or path.endswith('.pt'):
        return load_image(path, IMAGE_SHAPE).to(device)
    global _transform
    import numpy as np
    from PIL import Image
    from ..preprocess import ResizeCenterCropToTensor
    if _transform is None:
        _transform = ResizeCenterCropToTensor(64)
    arr = np.ascontiguousarray(np.array(Image.open(path).convert('RGB')))
    return _transform(torch.from_numpy(arr).unsqueeze(0).to(device))


def main(argv=None):
    """``python celeba19/sample.py model_path --cuda [...]``: writes ``sample_image.png`` and ``sample_attrs.txt`` (one
    line per sample: the attributes above 0.5, the format of celeba/sample.py); with --sweep one grid row per condition
    and ``sweep_attrs.txt``: per condition its label and the 18 mean attribute probabilities over its samples."""
    import argparse
    from ..sample_common import add_common_flags, need_cuda, save_image
    from .train import load_checkpoint
    parser = argparse.ArgumentParser()
    add_common_flags(parser)
    parser.add_argument('--condition-on-attrs', type=str, default=None, metavar='SPEC',
                        help='attributes to condition on, e.g. Male=1,Eyeglasses=0 (names or indices 0-17; a bare name is =1)')
    parser.add_argument('--condition-on-image', action='store_true', default=False,
                        help='condition on the image of --image-file (or a random one with --synthetic)')
    parser.add_argument('--sweep', action='store_true', default=False,
                        help='37 conditions in one launch: the prior, then every attribute at 0 and at 1')
    parser.add_argument('--mean', action='store_true', default=False,
                        help='decode the posterior mean instead of drawing (one sample per condition)')
    parser.add_argument('--seed', type=int, default=0, help='seed of the device noise stream [default: 0]')
    args = parser.parse_args(argv)
    row = parse_conditions(args.condition_on_attrs)            # refusals of the spec come before the device is needed
    if args.condition_on_image and not (args.image_file or args.synthetic):
        raise SystemExit('--condition-on-image needs --image-file or --synthetic (the CelebA dataset loader is out of scope)')
    if args.n_samples < 1:
        raise SystemExit('--n-samples must be at least 1')
    need_cuda(args)
    model = load_checkpoint(args.model_path, use_cuda=True)
    model.cuda().eval()
    image = None
    if args.condition_on_image:
        image = load_condition_image(args.image_file) if args.image_file else torch.rand((1,) + IMAGE_SHAPE)
    if args.sweep:
        state = sweep_states()
        for a, v in enumerate(row):                            # the named attributes stay fixed across the sweep
            if v != -1:
                state[:, a] = torch.where(state[:, a] == -1, torch.tensor(v, dtype=torch.int8), state[:, a])
        labels = sweep_labels()
    else:
        state = torch.tensor([row], dtype=torch.int8)
        labels = [args.condition_on_attrs or 'prior']
    C = state.shape[0]
    img_row = torch.zeros(C, dtype=torch.int32) if image is not None else None
    n = 0 if args.mean else args.n_samples
    out = generate(model, image=image, img_row=img_row, state=state, n_samples=n, seed=args.seed)
    lead = out['z'].shape[0]
    # one grid row per condition: [C, lead] images, condition-major
    grid = out['image'].permute(1, 0, 2, 3, 4).reshape((C * lead,) + IMAGE_SHAPE)
    save_image(grid, os.path.join(args.out_dir, 'sample_image.png'), nrow=lead if args.sweep else 8)
    probs = out['attrs'].permute(1, 0, 2).cpu()                # [C, lead, 18]
    with open(os.path.join(args.out_dir, 'sample_attrs.txt'), 'w') as fp:
        for c in range(C):
            for k in range(lead):
                fp.write('%s\n' % ','.join(tensor_to_attributes(probs[c, k])))
    if args.sweep:
        with open(os.path.join(args.out_dir, 'sweep_attrs.txt'), 'w') as fp:
            for c in range(C):
                fp.write('%s %s\n' % (labels[c], ' '.join('%.4f' % p for p in probs[c].mean(0).tolist())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
