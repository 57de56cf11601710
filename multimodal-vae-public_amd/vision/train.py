"""Drop-in for the reference's ``vision/train.py``: same CLI (--n-latents 250 --batch-size 50 --epochs 100
--annealing-epochs 20 --lr 1e-4 --log-interval 10 --cuda), same function names, log lines and checkpoint format.

    python multimodal-vae-public_amd/vision/train.py --cuda --synthetic

The reference text does not run.  What is built is its documented behaviour, with the defects that prevent running
repaired and the code that would run kept as written:

    :20-21   ``elbo_loss``'s signature names ``recon_rotated, rotated`` while the body reads ``recon_watermark,
             watermark`` (:48) -- the signature is (recon_image, image, recon_gray, gray, recon_edge, edge, recon_mask,
             mask, recon_obscured, obscured, recon_watermark, watermark, mu, logvar, annealing_factor=1.)
    :57      ELBO = mean(BCE / 6 + annealing_factor * KLD)
    :139,157,302,324,327,378  ``datasets`` / ``tqdm`` never imported, the loop unpacks ``rotated_image``, ``test()`` passes
             a stray ``batch_size`` and calls ``loss_function``, ``sys.maxint`` -- ``test()`` is one joint ``model(...)``
             plus ``elbo_loss`` at beta 1 and writes six ``reconstruction_%d.png`` under ``results/<modality>/``
    KEPT :242  the gray term's KL is taken on ``(gray_mu, joint_logvar)``: that line runs, so it is built as written.  Its
             gradient reaches the joint term's ``logvar`` (and through it all six encoders), not the gray call's.

The per-batch body exists twice: ``train_step`` is the reference's loop body (:183-288) run eagerly -- seven ``model()``
calls, seven ``elbo_loss`` -- and ``fused_step`` computes the same step batched (each encoder trunk once, one PoE
launch for the seven terms, each decoder once on 7B rows, ONE segmented BCE launch for the 42 image terms).  ``--step``
selects one; ``fused`` is the default because it measured faster (9.9 against 28.5 ms per step at B = 50, D = 250:
profiles/vision_step.txt).

Without ``--synthetic`` the loaders are ``datasets.CelebVisionLoader`` over ``--data-dir`` ('train' shuffled, 'val' not;
vision/train.py:138-144) with the watermark of ``--watermark-file``.  The edge folder is written by ``vision/setup.py edge``
(Canny on HIP kernels), or not needed at all with ``--edge canny`` (the loader derives the edges per batch on the GPU);
the mask folder is written by the reference's ``vision/setup.py`` (dlib face masks), which is out of scope here.  When a
folder is missing the script says so and exits."""
import os
import sys

if __package__ in (None, ''):      # executed as a script, like the reference (`python train.py`)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.vision'

import torch  # noqa: E402

from .. import kernels as K  # noqa: E402
from .. import layers as L  # noqa: E402
from ..functional import binary_cross_entropy_with_logits  # noqa: E402,F401
from ..functional import elbo_loss_vision as elbo_loss  # noqa: E402
from ..functional import PoEFn, _GroupMeansFn, _KlRowsFn, vision_bce_rows  # noqa: E402
from ..optim import FusedAdam  # noqa: E402
from ..sample_common import save_image  # noqa: E402
from ..train_common import AverageMeter, make_load_checkpoint, reference_parser, save_checkpoint  # noqa: E402,F401
from .model import MODALITIES, MVAE, N_CHANNELS  # noqa: E402

load_checkpoint = make_load_checkpoint(MVAE)
N_TERMS = 1 + len(MODALITIES)       # the joint term, then one per modality (vision/train.py:186-214)
KEEP = 0.9                          # Dropout(p=0.1), vision/model.py:136


class SyntheticLoader(object):
    """len() / iteration surface of the reference's DataLoader (vision/train.py:138-144): six random tensors
    [B, C, 64, 64] in [0, 1], C = 3, 1, 1, 1, 3, 3."""
    def __init__(self, batch_size, n_batches, seed, device):
        self.batch_size, self.n, self.seed, self.device = batch_size, n_batches, seed, device
        self.dataset = range(batch_size * n_batches)

    def __len__(self):
        return self.n

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        for _ in range(self.n):
            yield tuple(torch.rand(self.batch_size, N_CHANNELS[m], 64, 64, generator=g).to(self.device) for m in MODALITIES)


def _call_noise(noise, call):
    """(eps, dropout_masks) of ``model()`` call ``call`` from the replayed noise: a list of seven dicts
    {'eps': [B, D], 'masks': six [B, 512] keep-masks or None}; (None, None) when the device stream draws."""
    if noise is None:
        return None, None
    return noise[call]['eps'], noise[call]['masks']


def _begin(model, optimizer):
    if optimizer is not None:
        optimizer.zero_grad()
    else:                           # parity runs without an update: the gradients are left in p.grad
        for p in model.parameters():
            p.grad = None


def train_step(model, optimizer, batch6, annealing_factor, noise=None):
    """The reference's loop body (vision/train.py:183-288): the joint call, one call per modality, seven ``elbo_loss``,
    ``backward()``, Adam.  The gray term's KL is taken on (gray_mu, joint_logvar) as :242 writes it, so the joint
    ``logvar`` receives that term's KL gradient.  ``batch6``: (image, gray, edge, mask, obscured, watermark).
    Returns (loss, the seven terms), detached device tensors."""
    _begin(model, optimizer)
    outs = []
    for call in range(N_TERMS):
        eps, masks = _call_noise(noise, call)
        inputs = {m: batch6[i] for i, m in enumerate(MODALITIES) if call == 0 or call == i + 1}
        outs.append(model(eps=eps, dropout_masks=masks, **inputs))
    joint_logvar = outs[0][7]
    terms = []
    for call, out in enumerate(outs):
        pairs = [v for pair in zip(out[:6], batch6) for v in pair]
        logvar = joint_logvar if call == 1 + MODALITIES.index('gray') else out[7]          # :242, as written
        terms.append(elbo_loss(*pairs, out[6], logvar, annealing_factor=annealing_factor))
    train_loss = terms[0]
    for t in terms[1:]:
        train_loss = train_loss + t
    train_loss.backward()
    if optimizer is not None:
        optimizer.step()
    return train_loss.detach(), torch.stack([t.detach() for t in terms])


class _DropoutFanFn(torch.autograd.Function):
    """h [B, N], keep-masks [G, B, N] -> [G * B, N]: the G independent Dropout draws of one activation."""

    @staticmethod
    def forward(ctx, h, masks):
        h = h.contiguous()
        G, B, N = masks.shape
        out = torch.empty(G * B, N, dtype=torch.float32, device=h.device)
        K.dropout_fanout_fwd(h, masks, out, 1.0 / KEEP)
        ctx.save_for_backward(masks)
        return out

    @staticmethod
    def backward(ctx, g):
        masks, = ctx.saved_tensors
        dh = torch.empty(masks.shape[1], masks.shape[2], dtype=torch.float32, device=g.device)
        K.dropout_fanin_bwd(g.contiguous(), masks, dh, 1.0 / KEEP)
        return dh, None


_TERM_MASKS = {}


def _term_masks(device):
    """The experts of the seven terms over twelve heads (six joint-call heads, then six single-call heads): the joint
    term takes heads 0..5, term i the single-call head of encoder i; the prior is built into the launch."""
    m = _TERM_MASKS.get(str(device))
    if m is None:
        n = len(MODALITIES)
        m = torch.tensor([(1 << n) - 1] + [1 << (n + i) for i in range(n)], dtype=torch.int32, device=device)
        _TERM_MASKS[str(device)] = m
    return m


def fused_step(model, optimizer, batch6, annealing_factor, noise=None):
    """The same step as ``train_step`` -- the same loss, gradients, BatchNorm running statistics and
    ``num_batches_tracked`` -- batched: each encoder's trunk runs once with two running-statistics updates (the reference
    calls it twice on the same input), its two Dropout draws are fanned out and the head Linear runs on both; one PoE
    launch forms the seven terms' posteriors from the twelve heads; each decoder runs once on [7B, D] as seven BatchNorm
    groups in the reference's call order; one segmented BCE launch covers the 42 image terms.  The gray term's KL is
    taken on (gray_mu, joint_logvar), as in ``train_step``.  Runs under autograd, no graph capture, one stream."""
    _begin(model, optimizer)
    model.finalize()
    B, D = batch6[0].shape[0], model.n_latents
    dev = batch6[0].device
    heads_joint, heads_single = [], []
    for i, enc in enumerate(model.encoders()):
        h = L.run_plan(enc.trunk_plan(), batch6[i], bn_updates=2, training=True)
        if noise is None:
            masks = model.device_bernoulli(KEEP, 2, B, 512)
        else:
            masks = torch.stack((noise[0]['masks'][i], noise[i + 1]['masks'][i])).float().contiguous()
        h2 = L.run_plan(enc.head_plan(), _DropoutFanFn.apply(h, masks), training=True)
        heads_joint.append(h2[:B]); heads_single.append(h2[B:])
    eps = model.device_randn(N_TERMS, B, D) if noise is None else torch.stack([nz['eps'] for nz in noise]).contiguous()
    mu, logvar, z, _ = PoEFn.apply((_term_masks(dev), eps, model.POE_VARIANT, D), *(heads_joint + heads_single))
    zf = z.reshape(N_TERMS * B, D)
    recons = [dec.run(zf, groups=N_TERMS) for dec in model.decoders()]
    bce = vision_bce_rows(recons, batch6)
    gray = 1 + MODALITIES.index('gray')
    kl_logvar = torch.cat((logvar[:gray], logvar[:1], logvar[gray + 1:]))      # vision/train.py:242
    kl = _KlRowsFn.apply(mu.reshape(N_TERMS * B, D), kl_logvar.reshape(N_TERMS * B, D))
    train_loss, terms = _GroupMeansFn.apply([1.0, float(annealing_factor)], N_TERMS, bce, kl)
    train_loss.backward()
    if optimizer is not None:
        optimizer.step()
    return train_loss.detach(), terms.detach()


STEPS = {'eager': train_step, 'fused': fused_step}
DEFAULT_STEP = 'fused'      # measured faster beyond the spread at B = 50, D = 250: profiles/vision_step.txt


def parser():
    p = reference_parser('vision')
    p.add_argument('--step', choices=sorted(STEPS), default=DEFAULT_STEP,
                   help="'eager': the reference's loop body, seven model() calls; 'fused': the same step batched "
                        "[default: %s]" % DEFAULT_STEP)
    p.add_argument('--watermark-file', type=str, default='./watermark.png',
                   help='the image with an alpha channel pasted onto the colour image for the watermark modality '
                        '[default: ./watermark.png]')
    add_edge_flag(p)
    return p


def add_edge_flag(p):
    p.add_argument('--edge', choices=['folder', 'canny'], default='folder',
                   help="'folder': read the edge folder vision/setup.py edge wrote; 'canny': derive the edge modality "
                        "from the colour image on the GPU, no edge folder needed [default: folder]")


def check_data(args):
    """Without --synthetic: exit with what is missing under --data-dir, or when --watermark-file is."""
    from .datasets import missing_data
    missing = missing_data(args.data_dir, edge=args.edge)
    if missing:
        raise SystemExit('the vision data set is not under --data-dir %s: missing %s.  The edge folder is written by '
                         '`vision/setup.py edge in_dir out_dir` of this repository (Canny on HIP kernels), or pass '
                         '--edge canny and the loader derives the edges on the GPU.  Building the mask folder '
                         "(the reference's vision/setup.py mask: dlib face masks) is out of scope here: run the "
                         "reference's setup.py for it first, or run with --synthetic"
                         % (args.data_dir, ', '.join(missing)))
    if not os.path.isfile(args.watermark_file):
        raise SystemExit('the watermark image %s is missing: name one with --watermark-file (an image with an alpha '
                         'channel), or run with --synthetic' % args.watermark_file)


def main(argv=None):
    args = parser().parse_args(argv)
    if not args.synthetic:
        check_data(args)
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit('this drop-in runs the MVAE step as HIP kernels: pass --cuda on a ROCm GPU box '
                         '(the CPU path is the reference itself)')
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    results = os.path.join(args.out_dir, 'results')
    for d in [args.out_dir, results] + [os.path.join(results, m) for m in MODALITIES]:
        if not os.path.isdir(d):
            os.makedirs(d)
    if args.synthetic:
        train_loader = SyntheticLoader(args.batch_size, args.steps_per_epoch, 1234, device)
        test_loader = SyntheticLoader(args.batch_size, max(1, args.steps_per_epoch // 10), 4321, device)
    else:
        from .datasets import CelebVisionLoader
        train_loader = CelebVisionLoader('train', args.data_dir, args.batch_size, True, device, seed=1234,
                                         watermark_path=args.watermark_file, edge=args.edge)
        test_loader = CelebVisionLoader('val', args.data_dir, args.batch_size, False, device,
                                        watermark_path=args.watermark_file, edge=args.edge)
        for name, loader in (('train', train_loader), ('val', test_loader)):
            if len(loader) == 0:
                raise SystemExit('%s lists no image of the %r partition'
                                 % (os.path.join(args.data_dir, 'Eval/list_eval_partition.txt'), name))
    N_mini_batches = len(train_loader)

    model = MVAE(args.n_latents, use_cuda=True)
    model.cuda(device)
    optimizer = FusedAdam(model.parameters(), lr=args.lr)
    step = STEPS[args.step]

    def train(epoch):
        model.train()
        train_loss_meter = AverageMeter()
        pending = []          # device-side losses; read back only at the log interval
        for batch_idx, batch6 in enumerate(train_loader):
            if epoch < args.annealing_epochs:
                annealing_factor = (float(batch_idx + (epoch - 1) * N_mini_batches + 1) /
                                    float(args.annealing_epochs * N_mini_batches))
            else:
                annealing_factor = 1.0
            loss, _ = step(model, optimizer, batch6, annealing_factor)
            pending.append((loss, len(batch6[0])))
            if batch_idx % args.log_interval == 0:
                for v, n in zip(torch.stack([q[0] for q in pending]).tolist(), [q[1] for q in pending]):
                    train_loss_meter.update(v, n)
                pending = []
                print('Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f}\tAnnealing Factor: {:.3f}'.format(
                    epoch, batch_idx * len(batch6[0]), len(train_loader.dataset),
                    100. * batch_idx / len(train_loader), train_loss_meter.avg, annealing_factor))
        if pending:
            for v, n in zip(torch.stack([q[0] for q in pending]).tolist(), [q[1] for q in pending]):
                train_loss_meter.update(v, n)
        print('====> Epoch: {}\tLoss: {:.4f}'.format(epoch, train_loss_meter.avg))

    def test(epoch):
        model.eval()
        test_loss = 0
        with torch.no_grad():
            for batch_idx, batch6 in enumerate(test_loader):
                out = model(*batch6)            # for ease, only compute the joint loss (vision/train.py:321)
                pairs = [v for pair in zip(out[:6], batch6) for v in pair]
                test_loss += elbo_loss(*pairs, out[6], out[7]).item()
                if batch_idx == 0:
                    n = min(len(batch6[0]), 8)
                    for m, x, logits in zip(MODALITIES, batch6, out[:6]):
                        logits = logits[:n].contiguous()
                        recon = torch.empty_like(logits)
                        K.sigmoid_fwd(logits, recon)
                        save_image(torch.cat([x[:n], recon]), os.path.join(results, m, 'reconstruction_%d.png' % epoch),
                                   nrow=n)
        test_loss /= len(test_loader)
        print('====> Test Loss: {:.4f}'.format(test_loss))
        return test_loss

    best_loss = sys.maxsize
    for epoch in range(1, args.epochs + 1):
        train(epoch)
        loss = test(epoch)
        is_best = loss < best_loss
        best_loss = min(loss, best_loss)
        save_checkpoint({
            'state_dict': model.state_dict(),
            'best_loss': best_loss,
            'n_latents': args.n_latents,
            'optimizer': optimizer.state_dict(),
        }, is_best, folder=args.out_dir)


if __name__ == "__main__":
    main()
