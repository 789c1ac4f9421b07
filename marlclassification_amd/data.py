"""Input pipeline of the training driver: image folders are decoded on the
host to **uint8** ``[C, H, W]`` tensors (RGB forced, like the reference's ``my_pil_loader``,
data/datasets.py:17-22) and uploaded as uint8; ``ToTensor`` (x / 255) runs inside the HIP
gather kernel.  A synthetic dataset of the same interface serves benchmarks and smoke runs
(no dataset can be downloaded here)."""

import os
from typing import Dict, List, Optional, Tuple

import torch as th
from torch.utils.data import Dataset


class SyntheticImages(Dataset):
    """Uniform random uint8 images with random labels: shapes only."""

    def __init__(self, n: int, channels: int, size: int, nb_class: int, seed: int = 0) -> None:
        g = th.Generator().manual_seed(seed)
        self.x = th.randint(0, 256, (n, channels, size, size), dtype=th.uint8, generator=g)
        self.y = th.randint(0, nb_class, (n,), generator=g)
        self.class_to_idx: Dict[str, int] = {str(i): i for i in range(nb_class)}

    def __len__(self) -> int:
        return self.x.shape[0]

    def __getitem__(self, i: int) -> Tuple[th.Tensor, th.Tensor]:
        return self.x[i], self.y[i]


class ImageFolderU8(Dataset):
    """``root/<class>/<image>`` -> (uint8 [3, H, W], label); every image must have the
    configured side (the reference assumes square, equally sized images)."""

    EXT = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")

    def __init__(self, root: str, img_size: int = 0) -> None:
        from PIL import Image  # host-side decode only

        self._Image = Image
        self._img_size = img_size  # > 0: every image must be img_size x img_size
        classes = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
        self.class_to_idx = {c: i for i, c in enumerate(classes)}
        self.items: List[Tuple[str, int]] = []
        for c in classes:
            for f in sorted(os.listdir(os.path.join(root, c))):
                if f.lower().endswith(self.EXT):
                    self.items.append((os.path.join(root, c, f), self.class_to_idx[c]))

    def __len__(self) -> int:
        return len(self.items)

    def __getitem__(self, i: int) -> Tuple[th.Tensor, th.Tensor]:
        import numpy as np

        path, label = self.items[i]
        with open(path, "rb") as f:
            img = self._Image.open(f).convert("RGB")
        arr = th.from_numpy(np.asarray(img).copy())  # [H, W, 3] uint8
        if self._img_size and (arr.shape[0] != self._img_size or arr.shape[1] != self._img_size):
            raise ValueError(f"{path}: {arr.shape[1]}x{arr.shape[0]} image, --img-size is {self._img_size}")
        return arr.permute(2, 0, 1).contiguous(), th.tensor(label)


class DevicePrefetcher:
    """Double-buffered host -> device upload.  The reference moves every batch
    synchronously at the top of the iteration (training/trainer.py:67-68) behind a pin_memory
    DataLoader (train.py:91-107); here batch i+1 is copied (uint8: a quarter of the fp32 bytes,
    ToTensor runs in the gather kernel) from pinned staging memory on a COPY stream while batch
    i trains, and the compute stream only waits for the copy's event.

    ``augment``, ``mix`` (with ``nb_class``), ``color``, ``normalize`` and ``generator`` (a generator of ``device``):
    the policies of ``_batch``, which makes every yielded batch of the uploaded one (``rows`` None) on the compute
    stream, behind the wait on the copy's event.  All None: exactly the code above."""

    def __init__(self, loader, device: th.device, augment=None, generator=None, mix=None,
                 nb_class: Optional[int] = None, normalize=None, color=None) -> None:
        self.loader = loader
        self.device = th.device(device)
        self.normalize = _normalize_spec(normalize)
        self.mix, self.nb_class = mix, _mix_classes(mix, nb_class)
        self.augment = _no_mixed_warp(augment, mix)
        self.color = color
        self.generator = _device_generator(_first_policy(mix, augment, color), generator, self.device)

    def _upload(self, batch, stream):
        if batch is None:
            return None
        x, y = batch
        if not x.is_pinned():
            x = x.pin_memory()
        if not y.is_pinned():
            y = y.pin_memory()
        with th.cuda.stream(stream):
            xd = x.to(self.device, non_blocking=True)
            yd = y.to(self.device, non_blocking=True)
        ev = th.cuda.Event()
        ev.record(stream)
        return xd, yd, ev, (x, y)  # keep the pinned staging tensors alive until the copy ran

    def __iter__(self):
        copy_stream = th.cuda.Stream(device=self.device)
        it = iter(self.loader)
        nxt = self._upload(next(it, None), copy_stream)
        while nxt is not None:
            xd, yd, ev, _host = nxt
            nxt = self._upload(next(it, None), copy_stream)  # overlaps with the step below
            cur = th.cuda.current_stream(self.device)
            cur.wait_event(ev)
            xd.record_stream(cur)
            yd.record_stream(cur)
            yield _batch(self.augment, self.mix, self.nb_class, self.color, self.normalize, self.generator, xd, None, yd)

    def __len__(self) -> int:
        return len(self.loader)


def _device_generator(policy, generator, device: th.device):
    """the generator a loader draws ops from: the caller's, or (policy without one) a fresh one of the device, seed 0"""
    if policy is None or generator is not None:
        return generator
    return th.Generator(device=device).manual_seed(0)


def _first_policy(*policies):
    """the first policy that is given: what decides whether a loader needs a generator"""
    return next((p for p in policies if p is not None), None)


def _no_mixed_warp(augment, mix):
    """the augment policy of a loader; together with a mix policy it may not resample"""
    if mix is not None and augment is not None and augment.has_warp:
        raise ValueError(f'augment "{augment.spec}" with a mix policy: mixing warped views is not built '
                         "(marl_batch_mix remaps indices; rotate / scale / stretch resample)")
    return augment


def _augmented(policy, generator, x: th.Tensor, rows):
    """``augment.apply`` of ``x[rows]`` (``rows`` None: ``x`` itself) under freshly drawn ops - ``warp.apply`` under
    freshly drawn ops and matrices for a policy that resamples; a policy that turns images refuses non-square ones
    before anything is enqueued"""
    from . import augment as _augment

    policy.check_size(x.shape[-2], x.shape[-1])
    batch = x.shape[0] if rows is None else rows.shape[0]
    if policy.has_warp:
        from . import warp as _warp

        ops, mats = policy.draw_warp(batch, generator, size=(x.shape[-2], x.shape[-1]))
        return _warp.apply(x, rows, mats, ops, pad_mode=policy.pad_mode, fill=policy.fill)
    ops = policy.draw(batch, generator, size=(x.shape[-2], x.shape[-1]))
    return _augment.apply(x, rows, ops, pad_mode=policy.pad_mode, fill=policy.fill)


def _normalize_spec(normalize):
    """the transform of a loader: a ``transforms.Spec`` (or its spelling; "dataset" must be resolved before), or None"""
    from . import transforms as _transforms

    return _transforms.resolve(normalize)


def _normalized(spec, x: th.Tensor, rows):
    """``transforms.apply`` of ``x[rows]`` (``rows`` None: ``x`` itself) - the statistics are those of the batch as it is
    handed to the episode; ``spec`` None: ``x`` as it is (``rows`` is then None too)"""
    if spec is None:
        return x
    from . import transforms as _transforms

    return _transforms.apply(x, rows, spec)


def _finished(color, spec, generator, x: th.Tensor, rows):
    """the last steps of a batch: ``color.apply`` of ``x[rows]`` (``rows`` None: ``x`` itself) under parameters drawn
    now - the last draws of a batch - then ``_normalized``; a ``user-*`` transform of uint8 images rides the colour
    launch (``out_form="norm"``), a statistic transform takes the statistics of the jittered batch.  ``color`` None:
    ``_normalized`` alone"""
    if color is None:
        return _normalized(spec, x, rows)
    from . import color as _color
    from . import transforms as _transforms

    batch = x.shape[0] if rows is None else rows.shape[0]
    params = color.draw(batch, generator)
    records = _transforms.stats(x, rows) if color.needs_stats and batch > 0 else None
    if spec is not None and spec.is_user and x.dtype == th.uint8:
        return _color.apply(x, rows, params, records, out_form="norm", normalize=spec)
    return _normalized(spec, _color.apply(x, rows, params, records), None)


def _mix_classes(policy, nb_class) -> Optional[int]:
    if policy is not None and (isinstance(nb_class, bool) or not isinstance(nb_class, int) or nb_class < 1):
        raise ValueError(f"a mixing loader needs nb_class (the width of the target distributions), got {nb_class!r}")
    return nb_class


def _mixed(augment, policy, generator, x: th.Tensor, rows, y: th.Tensor, nb_class: int):
    """``(mix.apply of x[rows], primary labels, target distributions)`` under freshly drawn ops (``augment``, may be
    None) and a freshly drawn mix, in this order from one generator; ``y`` are the labels of the batch"""
    from . import mix as _mix

    h, w = x.shape[-2], x.shape[-1]
    batch = x.shape[0] if rows is None else rows.shape[0]
    ops, pad_mode, fill = None, "reflect", 0
    if augment is not None:
        augment.check_size(h, w)
        ops, pad_mode, fill = augment.draw(batch, generator, size=(h, w)), augment.pad_mode, augment.fill
    m = policy.draw(batch, generator, size=(h, w))
    out = _mix.apply(x, rows, ops, m, pad_mode=pad_mode, fill=fill)
    return out, _mix.primary_labels(y, m, h, w), _mix.soft_targets(y, m, h, w, nb_class)


def _batch(augment, mix, nb_class, color, normalize, generator, x: th.Tensor, rows, y: th.Tensor):
    """What a loader yields for one batch: ``x[rows]`` / ``y[rows]`` (``rows`` int64 ``[B]`` into a resident set; None:
    ``x`` and ``y`` are the batch, an uploaded one) under the loader's policies.  Every draw comes from ``generator``
    without a host synchronisation, in the order augment, mix, colour.

    ``augment`` (an ``augment.Policy``): the batch is ``augment.apply(x, rows, ops)`` - the gather with flips, quarter
    turns, shifts and erasing fused in, one launch that moves the bytes ``index_select`` moves - into a fresh tensor.  A
    policy with ``rotate`` / ``scale`` / ``stretch`` (``Policy.has_warp``) goes through ``warp.apply`` under
    ``Policy.draw_warp`` instead: the gather with the bilinear resampling fused in, still one launch.

    ``mix`` (a ``mix.Policy``, with ``nb_class``): the batch is mixed with a permutation of itself (CutMix / Mixup,
    ``mix.apply``: the views are the augmented ones, still one launch) and the result is ``(x, y_primary, Q)`` with the
    target distributions ``Q`` fp32 ``[B, nb_class]``, not ``(x, y)``.

    ``color`` (a ``color.Policy``): the batch is jittered by ``color.apply`` - brightness, contrast, saturation, hue as
    one colour matrix per image, one launch - after whatever gather made it and before the normalisation, under
    parameters drawn last.  Without an augment / mix policy it reads ``x`` through ``rows`` (no ``index_select``; the
    statistics contrast needs go through ``rows`` too); with a ``user-*`` ``normalize`` the same launch writes the
    normalised fp32 batch.

    ``normalize`` (a ``transforms.Spec``): the batch is standardised per image by ``transforms.apply`` and is fp32.
    Without an augment / mix policy it reads ``x`` through ``rows`` - the ``index_select`` disappears; with one, the
    batch the policy produced is normalised.

    All None: ``x`` itself, or ``x.index_select(0, rows)``."""
    labels = y if rows is None else y.index_select(0, rows)
    if mix is not None:
        xm, yp, q = _mixed(augment, mix, generator, x, rows, labels, nb_class)
        return _finished(color, normalize, generator, xm, None), yp, q
    if augment is not None:
        return _finished(color, normalize, generator, _augmented(augment, generator, x, rows), None), labels
    if color is not None or normalize is not None:  # (through rows: no index_select)
        return _finished(color, normalize, generator, x, rows), labels
    return (x if rows is None else x.index_select(0, rows)), labels


class _Stripe:
    """every k-th batch of a batch sampler (same order: the base sampler is re-iterated per stripe)"""

    def __init__(self, base, k: int, j: int) -> None:
        self.base, self.k, self.j = base, k, j

    def __iter__(self):
        for i, b in enumerate(self.base):
            if i % self.k == self.j:
                yield b

    def __len__(self) -> int:
        n = len(self.base)
        return (n - self.j + self.k - 1) // self.k if n > self.j else 0


class StripedLoader:
    """``stripes`` DataLoaders over one batch sampler, batch i from loader i % stripes, yielded in order.
    One DataLoader funnels every batch through ONE collate / pin-memory thread of the parent process:
    measured 12.4 k images/s (256 x 256 uint8) whether 6, 32 or 96 workers decode; k stripes have k such
    threads (profiles/r04_loader.json)."""

    def __init__(self, dataset, batch_sampler, workers: int, stripes: int, **kw) -> None:
        from torch.utils.data import DataLoader

        self.batch_sampler = batch_sampler
        stripes = max(1, min(stripes, max(1, workers)))
        per = max(1, workers // stripes) if workers > 0 else 0
        self.loaders = [DataLoader(dataset, batch_sampler=_Stripe(batch_sampler, stripes, j), num_workers=per,
                                   pin_memory=True, persistent_workers=per > 0,
                                   prefetch_factor=4 if per > 0 else None, **kw) for j in range(stripes)]

    def __iter__(self):
        its = [iter(dl) for dl in self.loaders]
        i = 0
        while True:
            b = next(its[i % len(its)], None)
            if b is None:
                return
            yield b
            i += 1

    def __len__(self) -> int:
        return len(self.batch_sampler)


class ResidentLoader:
    """The whole image set decoded ONCE and kept in HBM as uint8 (``[N, C, H, W]``); every
    later batch is a device-side row gather, so from the second pass on the input pipeline
    costs no host work at all.  The reference re-decodes every image every epoch behind 6
    DataLoader workers (train.py:91-107), which one MI355X out-runs (input
    pipeline); 288 GB of HBM hold e.g. all of AID (10 000 x 3 x 600 x 600 B = 10.8 GB) many
    times over.  With ``world > 1`` each rank decodes ``1/world`` of the images and the
    shards are exchanged with one all-gather, so the host work is not repeated per rank.

    ``batch_sampler`` yields lists of dataset indices (this rank's slice of every global
    batch, train.ShardedBatchSampler); ``indices`` is the set it draws from.

    ``augment``, ``mix`` (with ``nb_class``), ``color``, ``normalize`` (a ``transforms.Spec`` or its spelling) and
    ``generator`` (a generator of ``device``): the policies of ``_batch``, which makes every batch from the resident
    set and the batch's ``rows``; labels are gathered as before.  All None: exactly the ``index_select`` above."""

    def __init__(self, dataset, indices, batch_sampler, device, workers: int = 0,
                 rank: int = 0, world: int = 1, group=None, chunk: int = 16, augment=None, generator=None,
                 mix=None, nb_class: Optional[int] = None, normalize=None, color=None) -> None:
        self.normalize = _normalize_spec(normalize)
        self.color = color
        self.dataset, self.batch_sampler = dataset, batch_sampler
        self.indices = list(indices)
        self.device = th.device(device)
        self.workers, self.rank, self.world, self.group, self.chunk = workers, rank, world, group, chunk
        self._x = self._y = self._row_of = None
        self.fill_img_s = float("nan")
        self.mix, self.nb_class = mix, _mix_classes(mix, nb_class)
        self.augment = _no_mixed_warp(augment, mix)
        self.generator = _device_generator(_first_policy(mix, augment, color), generator, self.device)

    @staticmethod
    def nbytes(dataset, n: int) -> int:
        x, _ = dataset[0]
        return n * x.numel() * x.element_size()

    def _fill(self) -> None:
        from torch.utils.data import DataLoader

        n = len(self.indices)
        n_loc = -(-n // self.world)
        mine = self.indices[self.rank::self.world]
        mine = mine + [self.indices[-1]] * (n_loc - len(mine))  # equal shards for the all-gather
        chunks = [mine[i: i + self.chunk] for i in range(0, n_loc, self.chunk)]
        pin = self.device.type == "cuda"
        dl = DataLoader(self.dataset, batch_sampler=chunks, num_workers=self.workers, pin_memory=pin,
                        prefetch_factor=4 if self.workers > 0 else None)
        x_loc = y_loc = None
        at = 0
        import time

        t_first = None  # (fill_img_s: rate from the first chunk on - worker start-up excluded)
        for x, y in dl:
            if t_first is None:
                t_first, n_first = time.perf_counter(), x.shape[0]
            if x_loc is None:
                x_loc = th.empty((n_loc,) + tuple(x.shape[1:]), dtype=x.dtype, device=self.device)
                y_loc = th.empty((n_loc,), dtype=y.dtype, device=self.device)
            x_loc[at: at + x.shape[0]].copy_(x, non_blocking=pin)
            y_loc[at: at + x.shape[0]].copy_(y, non_blocking=pin)
            at += x.shape[0]
        assert at == n_loc
        if self.device.type == "cuda":
            th.cuda.synchronize(self.device)
        dt = time.perf_counter() - t_first if t_first is not None else 0.0
        self.fill_img_s = (n_loc - n_first) / dt if dt > 0 and n_loc > n_first else float("nan")
        if self.world > 1:
            import torch.distributed as dist

            # ONE [world * n_loc, ...] buffer filled in place: peak = (1 + 1 / world) x the image set
            x_all = th.empty((self.world * n_loc,) + tuple(x_loc.shape[1:]), dtype=x_loc.dtype, device=self.device)
            y_all = th.empty((self.world * n_loc,), dtype=y_loc.dtype, device=self.device)
            dist.all_gather_into_tensor(x_all, x_loc, group=self.group)
            dist.all_gather_into_tensor(y_all, y_loc, group=self.group)
            x_loc, y_loc = x_all, y_all
        # indices[j] was decoded by rank j % world as its (j // world)-th image
        j = th.arange(n)
        row_of = th.full((max(self.indices) + 1,), -1, dtype=th.long)
        row_of[th.tensor(self.indices, dtype=th.long)] = (j % self.world) * n_loc + j // self.world
        self._x, self._y, self._row_of = x_loc, y_loc, row_of.to(self.device)

    def __iter__(self):
        if self._x is None:
            self._fill()
        for batch in self.batch_sampler:
            rows = self._row_of[th.tensor(batch, dtype=th.long).to(self.device, non_blocking=True)]
            yield _batch(self.augment, self.mix, self.nb_class, self.color, self.normalize, self.generator, self._x,
                         rows, self._y)

    def __len__(self) -> int:
        return len(self.batch_sampler)
