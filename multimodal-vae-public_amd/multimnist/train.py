"""Drop-in for the reference's ``multimnist/train.py``: same CLI (--n-latents --batch-size --epochs
--annealing-epochs --lr --log-interval --lambda-image --lambda-text --cuda), same function names, log lines and
checkpoint format.  The per-batch body is the reference's own (multimnist/train.py:207-229) -- three ``model()``
calls, three ``elbo_loss``, ``backward()``, Adam -- run EAGERLY on the HIP modules with ``FusedAdam``: there is no
fused or captured MultiMNIST step.

    python multimodal-vae-public_amd/multimnist/train.py --cuda --synthetic

Without ``--synthetic`` the batches come from ``<data-dir>/multimnist/{training,test}.pt`` through
``datasets.MultiMNISTLoader`` (the split resident in HBM, ToTensor on the device).  The data set does not exist until
it is built: when the files are missing the script names the dataset builder's command and exits."""
import os
import sys

if __package__ in (None, ''):      # executed as a script, like the reference (`python train.py`)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.multimnist'

import torch  # noqa: E402

from ..functional import binary_cross_entropy_with_logits, cross_entropy  # noqa: E402,F401
from ..functional import elbo_loss_text as elbo_loss  # noqa: E402
from ..optim import FusedAdam  # noqa: E402
from ..train_common import AverageMeter, make_load_checkpoint, reference_parser, save_checkpoint  # noqa: E402,F401
from .model import FILL, MVAE, max_length  # noqa: E402

load_checkpoint = make_load_checkpoint(MVAE)


def synthetic_text(batch, generator):
    """Random MultiMNIST labels: 0-4 digits, FILL-padded (multimnist/utils.py:22-31 char_tensor)."""
    digits = torch.randint(0, 10, (batch, max_length), generator=generator)
    n = torch.randint(0, max_length + 1, (batch,), generator=generator)
    pos = torch.arange(max_length).unsqueeze(0)
    return torch.where(pos < n.unsqueeze(1), digits, torch.full_like(digits, FILL))


class SyntheticLoader(object):
    """len() / iteration surface of the reference's DataLoader (multimnist/train.py:168-176): random images
    [B, 1, 50, 50] in [0, 1] and random digit strings [B, 4] int64."""
    def __init__(self, batch_size, n_batches, seed, device, last_batch=0):
        self.batch_size, self.n, self.seed, self.device = batch_size, n_batches, seed, device
        self.last_batch = int(last_batch)
        self.dataset = range(batch_size * n_batches - (batch_size - self.last_batch if self.last_batch else 0))

    def __len__(self):
        return self.n

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        for i in range(self.n):
            bs = self.last_batch if (self.last_batch and i == self.n - 1) else self.batch_size
            image = torch.rand(bs, 1, 50, 50, generator=g)
            text = synthetic_text(bs, g)
            yield image.to(self.device), text.to(self.device)


def train_step(model, optimizer, image, text, lambda_image, lambda_text, annealing_factor):
    """The reference's loop body (multimnist/train.py:207-229).  Returns the step's loss (a 0-d device tensor)."""
    optimizer.zero_grad()
    model.attach_text_grads()       # the text stacks' gradients arrive through autograd: cleared arena views
    recon_image_1, recon_text_1, mu_1, logvar_1 = model(image, text)
    recon_image_2, recon_text_2, mu_2, logvar_2 = model(image)
    recon_image_3, recon_text_3, mu_3, logvar_3 = model(text=text)
    joint_loss = elbo_loss(recon_image_1, image, recon_text_1, text, mu_1, logvar_1,
                           lambda_image=lambda_image, lambda_text=lambda_text, annealing_factor=annealing_factor)
    image_loss = elbo_loss(recon_image_2, image, None, None, mu_2, logvar_2,
                           lambda_image=lambda_image, lambda_text=lambda_text, annealing_factor=annealing_factor)
    text_loss = elbo_loss(None, None, recon_text_3, text, mu_3, logvar_3,
                          lambda_image=lambda_image, lambda_text=lambda_text, annealing_factor=annealing_factor)
    train_loss = joint_loss + image_loss + text_loss
    train_loss.backward()
    optimizer.step()
    return train_loss.detach()


def _test_total(model, image, text):
    """multimnist/train.py:252-259: three calls, default lambdas, beta = 1."""
    r1 = model(image, text)
    r2 = model(image)
    r3 = model(text=text)
    return (elbo_loss(r1[0], image, r1[1], text, r1[2], r1[3])
            + elbo_loss(r2[0], image, None, None, r2[2], r2[3])
            + elbo_loss(None, None, r3[1], text, r3[2], r3[3]))


def parser():
    return reference_parser('multimnist')


def main(argv=None):
    args = parser().parse_args(argv)
    if not args.synthetic:
        from .datasets import MultiMNIST
        folder = os.path.join(args.data_dir, MultiMNIST.processed_folder)
        if not all(os.path.exists(os.path.join(folder, f)) for f in (MultiMNIST.training_file, MultiMNIST.test_file)):
            raise SystemExit('no MultiMNIST files under %s: run the dataset builder first (python %s --data-dir %s), '
                             'or run with --synthetic'
                             % (folder, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'datasets.py'), args.data_dir))
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit('this drop-in runs the MVAE step as HIP kernels: pass --cuda on a ROCm GPU box '
                         '(the CPU path is the reference itself)')
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    if not os.path.isdir(args.out_dir):
        os.makedirs(args.out_dir)
    if args.synthetic:
        train_loader = SyntheticLoader(args.batch_size, args.steps_per_epoch, 1234, device, last_batch=args.synthetic_last_batch)
        test_loader = SyntheticLoader(args.batch_size, max(1, args.steps_per_epoch // 10), 4321, device)
    else:
        from .datasets import MultiMNISTLoader
        train_loader = MultiMNISTLoader(args.data_dir, True, args.batch_size, True, device, seed=1234)
        test_loader = MultiMNISTLoader(args.data_dir, False, args.batch_size, False, device)
    N_mini_batches = len(train_loader)

    model = MVAE(args.n_latents)
    model.cuda(device)
    optimizer = FusedAdam(model.parameters(), lr=args.lr)

    def train(epoch):
        model.train()
        train_loss_meter = AverageMeter()
        pending = []          # device-side losses; read back only at the log interval
        for batch_idx, (image, text) in enumerate(train_loader):
            if epoch < args.annealing_epochs:
                annealing_factor = (float(batch_idx + (epoch - 1) * N_mini_batches + 1) /
                                    float(args.annealing_epochs * N_mini_batches))
            else:
                annealing_factor = 1.0
            loss = train_step(model, optimizer, image, text, args.lambda_image, args.lambda_text, annealing_factor)
            pending.append((loss, len(image)))
            if batch_idx % args.log_interval == 0:
                for v, n in zip(torch.stack([q[0] for q in pending]).tolist(), [q[1] for q in pending]):
                    train_loss_meter.update(v, n)
                pending = []
                print('Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f}\tAnnealing-Factor: {:.3f}'.format(
                    epoch, batch_idx * len(image), len(train_loader.dataset),
                    100. * batch_idx / len(train_loader), train_loss_meter.avg, annealing_factor))
        if pending:
            for v, n in zip(torch.stack([q[0] for q in pending]).tolist(), [q[1] for q in pending]):
                train_loss_meter.update(v, n)
        print('====> Epoch: {}\tLoss: {:.4f}'.format(epoch, train_loss_meter.avg))

    def test(epoch):
        model.eval()
        test_loss_meter = AverageMeter()
        with torch.no_grad():
            for image, text in test_loader:
                test_loss_meter.update(_test_total(model, image, text).item(), len(image))
        print('====> Test Loss: {:.4f}'.format(test_loss_meter.avg))
        return test_loss_meter.avg

    best_loss = sys.maxsize
    for epoch in range(1, args.epochs + 1):
        train(epoch)
        test_loss = test(epoch)
        is_best = test_loss < best_loss
        best_loss = min(test_loss, best_loss)
        save_checkpoint({
            'state_dict': model.state_dict(),
            'best_loss': best_loss,
            'n_latents': args.n_latents,
            'optimizer': optimizer.state_dict(),
        }, is_best, folder=args.out_dir)


if __name__ == "__main__":
    main()
