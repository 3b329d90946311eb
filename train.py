#!/usr/bin/env python3
"""Drop-in `train.py`: every flag of the reference (train.py:27-55) is kept verbatim; the step
loop (reference train.py:94-125) runs on the MI355X TrainEngine -- explicit HIP kernels for
forward/backward, one captured HIP graph per step, fused AdamW, metrics accumulated on the
device -- and shards each global minibatch data-parallel over the GPUs of the node with ONE RCCL
all-reduce of the flat gradient bucket per step.

    python train.py --dataset cifar10 --pos_encoding rope-axial --synthetic
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py \
        --dataset cifar10 --pos_encoding rope-mixed --batch_size 4096 --synthetic

Additions to the reference CLI: --synthetic (CIFAR/MNIST-shaped random batches generated on the
device: torchvision and the dataset downloads are unavailable offline), --steps_per_epoch,
--fp32 (exact-fp32 MFMA instead of the default bf16), --random_crop PAD / --hflip (RandomCrop(img_size, padding=PAD) /
RandomHorizontalFlip on the training images, drawn inside the embed kernel), --clip_grad MAX_NORM
(torch.nn.utils.clip_grad_norm_ between backward and the optimizer step, inside the captured step), --model_ema DECAY /
--model_ema_warmup (an exponential moving average of the weights, updated inside the captured step; every epoch also
evaluates the average and keeps its best checkpoint), --no_decay_norm_bias / --layer_decay D (AdamW parameter groups:
no weight decay on 1-d and position parameters, layer-wise learning-rate decay), --warmup_epochs E / --min_lr /
--lr_per_step (linear warm-up + cosine learning rate stepped every iteration, inside the captured step).  --batch_size is
the GLOBAL batch.
"""
import argparse
import csv
import math
import os
import sys
from datetime import datetime

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
for p in (REPO, os.path.join(REPO, "vit-rpe-rope_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def get_args(argv=None):
    parser = argparse.ArgumentParser(description='Vision Transformer Training (MI355X)')
    parser.add_argument('--log_dir', type=str, default='logs')
    parser.add_argument('--ckpt_dir', type=str, default='checkpoints')
    parser.add_argument('--dataset', type=str, default='mnist', choices=['mnist', 'cifar10'])
    parser.add_argument('--pos_encoding', type=str, default='absolute',
                        choices=['none', 'absolute', 'relative', 'polynomial', 'rope-axial', 'rope-mixed'])
    parser.add_argument('--rope_theta', type=float, default=100.0)
    parser.add_argument('--poly_degree', type=int, default=3)
    parser.add_argument('--poly_shared_heads', action='store_true', default=True)
    parser.add_argument('--no-poly_shared_heads', action='store_false', dest='poly_shared_heads')
    parser.add_argument('--batch_size', type=int, default=128)
    parser.add_argument('--epochs', type=int, default=25)
    parser.add_argument('--lr', type=float, default=0.001)
    parser.add_argument('--weight_decay', type=float, default=0.01)
    parser.add_argument('--img_size', type=int, default=32)
    parser.add_argument('--patch_size', type=int, default=4)
    parser.add_argument('--embed_dim', type=int, default=192)
    parser.add_argument('--depth', type=int, default=6)
    parser.add_argument('--num_heads', type=int, default=6)
    # additions
    parser.add_argument('--synthetic', action='store_true', help='dataset-shaped random batches generated on the device')
    parser.add_argument('--steps_per_epoch', type=int, default=0, help='0 = dataset size // batch_size')
    parser.add_argument('--fp32', action='store_true', help='exact-fp32 MFMA instead of bf16')
    parser.add_argument('--data_dir', type=str, default='./data',
                        help='directory holding the dataset in its binary format (CIFAR-10 binary batches / MNIST idx '
                             'files); it is loaded once into HBM as uint8 (no download: there is no network here)')
    parser.add_argument('--seed', type=int, default=0, help='seed of the per-epoch shuffle')
    # model options beyond the reference's CLI (its Block accepts them, its train.py never sets them); all off by default
    parser.add_argument('--qkv_bias', action='store_true', help='bias on the qkv projection')
    parser.add_argument('--drop', type=float, default=0.0, help='dropout rate behind attn.proj and inside the MLP')
    parser.add_argument('--attn_drop', type=float, default=0.0, help='dropout rate on the attention probabilities')
    parser.add_argument('--drop_path', type=float, default=0.0, help='stochastic depth: rate of the last block')
    parser.add_argument('--engine_extras', action='store_true',
                        help='run the TrainEngine on its per-Linear route, which has the four options above (opt-in: slower '
                             'than the fused default route)')
    # input augmentation of the training loop (the reference's pipeline has none); evaluation never augments
    parser.add_argument('--random_crop', type=int, default=0, metavar='PAD',
                        help='RandomCrop(img_size, padding=PAD) on the training images (0 = off)')
    parser.add_argument('--hflip', action='store_true', help='RandomHorizontalFlip() on the training images')
    parser.add_argument('--clip_grad', type=float, default=0.0, metavar='MAX_NORM',
                        help='clip_grad_norm_(model.parameters(), MAX_NORM) before every optimizer step (0 = off)')
    parser.add_argument('--model_ema', type=float, default=0.0, metavar='DECAY',
                        help='keep an exponential moving average of the weights with this decay, evaluate it every epoch '
                             'and save its best checkpoint (0 = off)')
    parser.add_argument('--model_ema_warmup', action='store_true',
                        help='ramp the decay up as min(DECAY, (1 + t) / (10 + t)) over the optimizer steps t')
    # AdamW parameter groups and the per-step schedule (TrainEngine.set_param_groups / set_lr_schedule); all off by default
    parser.add_argument('--no_decay_norm_bias', action='store_true',
                        help='no weight decay on 1-d parameters (norms, biases), the class token and the position parameters')
    parser.add_argument('--layer_decay', type=float, default=0.0, metavar='D',
                        help='layer-wise learning-rate decay: a layer k levels below the head trains at lr * D^k (0 = off)')
    parser.add_argument('--warmup_epochs', type=float, default=0.0, metavar='E',
                        help='linear warm-up over the first E epochs (a fraction is fine), then a per-step cosine')
    parser.add_argument('--min_lr', type=float, default=0.0, help='where the per-step cosine ends')
    parser.add_argument('--lr_per_step', action='store_true',
                        help='step the cosine every iteration on the device instead of once per epoch from the host')
    args = parser.parse_args(argv)
    if not (math.isfinite(args.layer_decay) and 0.0 <= args.layer_decay <= 1.0):
        parser.error("--layer_decay must be 0 (off) or a factor in (0, 1]")
    if not (math.isfinite(args.warmup_epochs) and 0.0 <= args.warmup_epochs < args.epochs):
        parser.error("--warmup_epochs must be a finite number in [0, --epochs)")
    if not (math.isfinite(args.min_lr) and 0.0 <= args.min_lr <= args.lr):
        parser.error("--min_lr must be in [0, --lr]")
    if args.min_lr > 0.0 and not (args.warmup_epochs > 0.0 or args.lr_per_step):
        parser.error("--min_lr belongs to the per-step schedule: it needs --warmup_epochs E or --lr_per_step")
    if not (math.isfinite(args.model_ema) and 0.0 <= args.model_ema < 1.0):
        parser.error("--model_ema must be 0 (off) or a decay in (0, 1)")
    if args.model_ema_warmup and args.model_ema == 0.0:
        parser.error("--model_ema_warmup needs --model_ema DECAY")
    if not (math.isfinite(args.clip_grad) and args.clip_grad >= 0.0):
        parser.error("--clip_grad must be a finite number >= 0")
    if not 0 <= args.random_crop <= args.img_size:
        parser.error(f"--random_crop must be in 0..--img_size ({args.img_size})")
    for name in ('drop', 'attn_drop', 'drop_path'):
        if not 0.0 <= getattr(args, name) < 1.0:
            parser.error(f"--{name} must be in [0, 1)")
    check_geometry(parser, args)
    return args


def check_geometry(parser, args):
    """The reference accepts any geometry ATen can run; here the attention kernels are compiled for a fixed set, so an
    unsupported combination of flags is refused up front with the list of what works (instead of a launch error)."""
    from vitpe import _lib
    if args.img_size % args.patch_size or args.embed_dim % args.num_heads:
        parser.error(f"--img_size {args.img_size} must be a multiple of --patch_size {args.patch_size} and --embed_dim "
                     f"{args.embed_dim} of --num_heads {args.num_heads}")
    n_tok = (args.img_size // args.patch_size) ** 2 + 1
    hd = args.embed_dim // args.num_heads
    dt = _lib.F32 if args.fp32 else _lib.BF16
    h = _lib.lib()
    if not (h.vitpe_fused_attention_supported(dt, n_tok, args.embed_dim, hd) or h.vitpe_attention_core_supported(dt, n_tok, hd)):
        ok = sorted({n for n in range(2, 300) if h.vitpe_attention_core_supported(dt, n, 32)})
        spans = []
        for n in ok:
            if spans and n == spans[-1][1] + 1:
                spans[-1][1] = n
            else:
                spans.append([n, n])
        # (at the fewest tokens every compiled head dimension fits; the widest heads in fp32 stop at fewer tokens)
        hds = [d for d in range(1, 513) if h.vitpe_attention_core_supported(dt, ok[0], d)]
        here = [d for d in hds if h.vitpe_attention_core_supported(dt, n_tok, d)]
        also = (f"; at {n_tok} tokens in {'fp32' if args.fp32 else 'bf16'}: head dimensions "
                + ", ".join(map(str, here)) if n_tok in ok and here != hds else "")
        parser.error(f"no attention kernel for {n_tok} tokens (img {args.img_size} / patch {args.patch_size}) with head "
                     f"dimension {hd} (--embed_dim {args.embed_dim} / --num_heads {args.num_heads}): supported head "
                     f"dimensions " + ", ".join(map(str, hds[:-1])) + f" and {hds[-1]}, token counts " +
                     ", ".join(f"{a}-{b}" for a, b in spans) +
                     " (e.g. 32/8 -> 17, 28/4 -> 50, 32/4 -> 65, 224/16 -> 197, 64/4 -> 257)" + also)
    if args.pos_encoding == 'polynomial' and not 0 <= args.poly_degree <= 7:
        parser.error("--poly_degree must be in 0..7 (the attention kernels tabulate the polynomial up to degree 7)")


DATASETS = {'mnist': dict(in_chans=1, num_classes=10, train=60000, test=10000),
            'cifar10': dict(in_chans=3, num_classes=10, train=50000, test=10000)}


class SyntheticBatches:
    """Dataset-shaped batches drawn on the device: images ~ N(0,1) (what Normalize produces,
    reference train.py:72,82), labels ~ U{0..9}; a fixed pool so a model can actually fit it."""

    def __init__(self, n_batches, batch, in_chans, img, num_classes, device, seed):
        g = torch.Generator(device=device).manual_seed(seed)
        pool = max(1, min(n_batches, 8))
        self.images = [torch.randn(batch, in_chans, img, img, generator=g, device=device) for _ in range(pool)]
        self.labels = [torch.randint(0, num_classes, (batch,), generator=g, device=device) for _ in range(pool)]
        self.n = n_batches

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            yield self.images[i % len(self.images)], self.labels[i % len(self.labels)]


class ResidentBatches:
    """One epoch's index batches over a `vitpe.data.ResidentDataset` (reference DataLoader(batch_size, shuffle=...),
    train.py:89-90, no drop_last): the loop hands the engine sample indices, the pixels never leave HBM.  Yields
    (idx, n_local, n_global) per GLOBAL batch; the ragged last batch is kept, as in the reference."""

    def __init__(self, dataset, global_batch, shuffle, seed, rank, world):
        self.ds, self.global_batch, self.shuffle, self.seed = dataset, global_batch, shuffle, seed
        self.rank, self.world = rank, world
        self.epoch = 0

    def __len__(self):
        return (len(self.ds) + self.global_batch - 1) // self.global_batch

    def __iter__(self):
        from vitpe.data import epoch_global_batches
        it = epoch_global_batches(len(self.ds), self.global_batch, self.epoch, self.seed, self.shuffle, self.rank,
                                  self.world, self.ds.device)
        self.epoch += 1
        return it


def get_dataset(args, info, per_rank_batch, device, rank, world=1):
    if not args.synthetic:
        from vitpe._lib import VitpeError
        from vitpe.data import ResidentDataset
        root = os.path.join(args.data_dir, {'cifar10': 'cifar-10-batches-bin', 'mnist': 'MNIST/raw'}[args.dataset])
        root = root if os.path.isdir(root) else args.data_dir
        try:
            tr = ResidentDataset.from_files(args.dataset, root, True, device, args.img_size)
            te = ResidentDataset.from_files(args.dataset, root, False, device, args.img_size)
        except VitpeError as e:
            raise SystemExit(f"{e}\nno dataset under {args.data_dir} (nothing is downloaded here): "
                             f"place the binary files there or re-run with --synthetic")
        return (ResidentBatches(tr, args.batch_size, True, args.seed, rank, world),
                ResidentBatches(te, args.batch_size, False, args.seed, rank, world))
    n_train = args.steps_per_epoch or info['train'] // args.batch_size
    n_test = max(1, min(n_train // 5, info['test'] // args.batch_size))
    mk = lambda n, seed: SyntheticBatches(n, per_rank_batch, info['in_chans'], args.img_size,  # noqa: E731
                                          info['num_classes'], device, seed)
    return mk(n_train, 1234 + rank), mk(n_test, 4321 + rank)


def train(engine, loader):
    """One epoch (reference train.py:94-125) -> (avg_loss, acc%) over ALL ranks' samples. No per-step host sync."""
    seen = 0
    resident = isinstance(loader, ResidentBatches)
    engine.attach_dataset(loader.ds if resident else None)
    for item in loader:
        if resident:
            idx, n_local, n_global = item
            engine.step_indexed(idx, n_global, n_valid=n_local)
            seen += n_global
        else:
            images, labels = item
            engine.step(images, labels)
            seen += images.shape[0] * engine.world
    loss_sum, correct = engine.read_metrics()      # global-batch means summed over the steps; all ranks' #correct
    return loss_sum / max(len(loader), 1), 100. * correct / max(seen, 1)


def test(engine, loader):
    """Evaluation (reference train.py:127-155): forward only on the same kernels, every sample of the set counted
    (ragged last batch included), totals summed over the ranks."""
    seen = 0
    acc = torch.zeros(2, device=engine.dev)
    resident = isinstance(loader, ResidentBatches)
    if not resident:
        engine.attach_dataset(None)
    for item in loader:
        if resident:
            idx, n_local, n_global = item
            engine.forward_indexed(idx, loader.ds)
            engine.eval_loss(n_local, acc, n_global)
            seen += n_global
        else:
            images, labels = item
            engine.forward_only(images, labels)     # (pads a short batch: images AND labels, like the resident path)
            engine.eval_loss(images.shape[0], acc, images.shape[0] * engine.world)
            seen += images.shape[0] * engine.world
    if engine.world > 1:
        torch.distributed.all_reduce(acc)
    loss_sum, correct = acc.tolist()
    return loss_sum / max(len(loader), 1), 100. * correct / max(seen, 1)


def engine_refusal(args):
    """The training loop here is the TrainEngine's, whose fused kernels have no qkv bias and no dropout: say so instead of
    training without what was asked for.  -> message, or None."""
    active = [f for f, on in (('--qkv_bias', args.qkv_bias), ('--drop', args.drop > 0), ('--attn_drop', args.attn_drop > 0),
                              ('--drop_path', args.drop_path > 0)) if on]
    if not active or args.engine_extras:
        return None
    return ("train.py: " + ", ".join(active) + " not supported by the TrainEngine training loop (no qkv bias, no dropout in "
            "its fused kernels); models.vit.VisionTransformer(..., qkv_bias=, drop_rate=, attn_drop_rate=, drop_path_rate=) "
            "runs them through the module path (torch autograd over torch.ops.vitpe.*).  --engine_extras trains them on the "
            "engine's per-Linear route")


def augment_refusal(args):
    """The crop and the flip are drawn inside the gather from the resident uint8 dataset; --synthetic has none.
    -> message, or None."""
    active = [f for f, on in (('--random_crop', args.random_crop > 0), ('--hflip', args.hflip)) if on]
    if not active or not args.synthetic:
        return None
    return ("train.py: " + ", ".join(active) + " cannot be combined with --synthetic: the augmentation runs inside the "
            "embed kernel's gather from the dataset resident in HBM, and the synthetic batches are fp32 tensors with no "
            "such dataset behind them; drop --synthetic (see --data_dir) or the augmentation flags")


def main(argv=None):
    args = get_args(argv)
    extras = engine_refusal(args) or augment_refusal(args)
    if extras:   # up front: before the dataset is loaded and the device touched
        raise SystemExit(extras)
    if not torch.cuda.is_available():
        raise SystemExit("train.py needs an MI355X: the HIP path is the only path (no CPU fallback)")
    from vitpe import ddp
    from vitpe.engine import TrainEngine
    from models.vit import VisionTransformer

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    device = torch.device('cuda', local_rank)
    rank, world, _ = ddp.init_from_env(device=device)
    if args.batch_size % world != 0:   # (epoch_global_batches cuts every global batch into `world` equal shares)
        raise SystemExit(f"--batch_size {args.batch_size} is not divisible by the world size {world}")
    lo, hi = ddp.shard_bounds(args.batch_size, rank, world)
    per_rank = hi - lo
    info = DATASETS[args.dataset]

    log_file = None
    if rank == 0:
        os.makedirs(args.log_dir, exist_ok=True)
        os.makedirs(args.ckpt_dir, exist_ok=True)
        timestamp = datetime.now().strftime('%Y%m%d_%H%M%S')
        log_file = f'{args.log_dir}/{args.dataset}_{args.pos_encoding}_{timestamp}.csv'
        with open(log_file, 'w', newline='') as f:
            csv.writer(f).writerow(['epoch', 'train_loss', 'train_acc', 'test_loss', 'test_acc', 'best_acc'] +
                                   (['ema_test_loss', 'ema_test_acc'] if args.model_ema > 0 else []))

    train_loader, test_loader = get_dataset(args, info, per_rank, device, rank, world)
    torch.manual_seed(0)
    model = VisionTransformer(img_size=args.img_size, patch_size=args.patch_size, in_chans=info['in_chans'],
                              num_classes=info['num_classes'], embed_dim=args.embed_dim, depth=args.depth,
                              num_heads=args.num_heads, pos_encoding=args.pos_encoding, rope_theta=args.rope_theta,
                              poly_degree=args.poly_degree, poly_shared_heads=args.poly_shared_heads,
                              qkv_bias=args.qkv_bias, drop_rate=args.drop, attn_drop_rate=args.attn_drop,
                              drop_path_rate=args.drop_path).to(device)   # (all off unless --engine_extras: refused above)
    engine = TrainEngine(model, per_rank, compute_dtype=torch.float32 if args.fp32 else torch.bfloat16,
                         lr=args.lr, weight_decay=args.weight_decay, extras=args.engine_extras)
    engine.broadcast_parameters(0)
    if args.random_crop > 0 or args.hflip:   # training steps only: test() runs forward_indexed, which never augments
        engine.set_augment(args.random_crop, args.hflip)
    engine.set_grad_clip(args.clip_grad)   # 0 = off
    use_ema = args.model_ema > 0
    if use_ema:   # after the broadcast: the average starts from the parameters every rank trains
        engine.set_ema(args.model_ema, warmup=args.model_ema_warmup)
    if args.no_decay_norm_bias or args.layer_decay > 0:   # every rank builds the same map
        from vitpe.optim import vit_param_groups
        engine.set_param_groups(vit_param_groups(model, no_decay=args.no_decay_norm_bias, layer_decay=args.layer_decay or None))
    per_step = args.warmup_epochs > 0 or args.lr_per_step
    if per_step:   # linear warm-up + cosine, stepped by the captured step itself: one schedule over the whole run
        steps_per_epoch = len(train_loader)
        warm = min(round(args.warmup_epochs * steps_per_epoch), args.epochs * steps_per_epoch - 1)
        engine.set_lr_schedule(args.lr, args.epochs * steps_per_epoch, warm, args.min_lr)

    best_acc = 0
    best_ema_acc = -1.0   # (the first epoch's average is always a checkpoint, also at 0 % on a toy run)
    for epoch in range(args.epochs):
        # CosineAnnealingLR(T_max=epochs), stepped per epoch (reference train.py:196,205)
        if not per_step:
            engine.set_lr(0.5 * args.lr * (1 + math.cos(math.pi * epoch / args.epochs)))
        train_loss, train_acc = train(engine, train_loader)
        test_loss, test_acc = test(engine, test_loader)
        ema_cols = []
        if use_ema:   # the same evaluation with the average swapped in for the weights (every rank: test() all-reduces)
            with engine.ema_weights():
                ema_test_loss, ema_test_acc = test(engine, test_loader)
                if rank == 0 and ema_test_acc > best_ema_acc:   # (inside the context model.state_dict() is the average)
                    best_ema_acc = ema_test_acc
                    torch.save(model.state_dict(), f'{args.ckpt_dir}/{args.dataset}_{args.pos_encoding}_best_ema.pth')
            ema_cols = [ema_test_loss, ema_test_acc]
        if rank == 0:
            print(f'\nEpoch: {epoch + 1}/{args.epochs}')
            if test_acc > best_acc:
                best_acc = test_acc
                torch.save(model.state_dict(), f'{args.ckpt_dir}/{args.dataset}_{args.pos_encoding}_best.pth')
            with open(log_file, 'a', newline='') as f:
                csv.writer(f).writerow([epoch + 1, train_loss, train_acc, test_loss, test_acc, best_acc] + ema_cols)
            print(f'Train Loss: {train_loss:.4f}, Train Acc: {train_acc:.2f}%')
            print(f'Test Loss: {test_loss:.4f}, Test Acc: {test_acc:.2f}%')
            print(f'Best Test Acc: {best_acc:.2f}%')
            if use_ema:
                print(f'EMA Test Loss: {ema_test_loss:.4f}, EMA Test Acc: {ema_test_acc:.2f}%')
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
