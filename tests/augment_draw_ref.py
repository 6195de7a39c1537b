"""What the device draws of TwoViewAugmenter(device_draws=True) are checked against, on the CPU:

  * a pure-Python Philox4x32-10 and the uniforms include/peclr_hip.h defines from it;
  * `Replay`, a generator whose .uniform(a, b) returns a + (b - a) * u for the next uniform the kernel used, so that
    TwoViewAugmenter.sample_view -- the host path, pinned to the reference by tests/golden/g9_augment_params.json -- computes
    the view of the same draws;
  * the inputs of the GPU cases and the FRAGILE pairs: (view, sample) for which a value sample_view truncates lies within 2^-10
    of an integer, where the summation order of a float32 mean (which torch does not specify) may decide the truncation.
"""
import math

import numpy as np
import torch

M32 = 0xFFFFFFFF
SLOTS = ("angle", "margin", "jitter_x", "jitter_y", "h", "s", "a", "b")
RECIPE = {"color_jitter": True, "random_crop": True, "rotate": True, "crop": True, "resize": True}
FRAGILE_EPS = 2.0 ** -10


def philox4x32_10(counter, key):
    """Salmon et al., SC'11: ten rounds, the key bumped by the Weyl constants before every round but the first."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def unit(a, b):
    """Python's random(): 53 bits of two 32-bit words."""
    return ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0


def uniforms(seed, call, v, i):
    """The eight uniforms of (view v, sample i) at call number `call`, in slot order."""
    out = []
    for k in range(4):
        x, y, z, w = philox4x32_10((i, 4 * v + k, call & M32, (call >> 32) & M32), (seed & M32, (seed >> 32) & M32))
        out += [unit(x, y), unit(z, w)]
    return out


def uniforms_table(seed, call, b, n_views=2):
    return np.array([[uniforms(seed, call, v, i) for i in range(b)] for v in range(n_views)], dtype=np.float64)


class Replay:
    """Stands in for `random`: hands sample_view the kernel's uniforms, slot by slot, in the order it draws them."""

    def __init__(self, u8, flags):
        order = ([0] if flags.get("rotate") else []) + ([1] if flags.get("random_crop") else []) \
            + ([2, 3] if flags.get("crop") else []) + ([4, 5, 6, 7] if flags.get("color_jitter") else [])
        self.us = [float(u8[s]) for s in order]
        self.at = 0

    def uniform(self, a, b):
        u = self.us[self.at]
        self.at += 1
        return a + (b - a) * u

    def getrandbits(self, n):
        raise AssertionError("the recipe flags draw no bits")


def make_inputs(sizes, seed, with_images=True):
    """Hand centres uniform in the middle 40 % of the image, joints spread +- 17.5 % of the side around them, from a seeded
    torch.Generator.  -> (list of HWC uint8 images or None, joints [B,21,3] float32)."""
    g = torch.Generator().manual_seed(seed)
    joints, images = [], []
    for h, w in sizes:
        side = torch.tensor([w, h], dtype=torch.float32)
        centre = (0.3 + 0.4 * torch.rand(2, generator=g)) * side
        xy = centre + (torch.rand(21, 2, generator=g) * 2 - 1) * 0.175 * side
        joints.append(torch.cat([xy, torch.rand(21, 1, generator=g)], 1))
        if with_images:
            images.append(torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8))
    return (images if with_images else None), torch.stack(joints)


def host_views(joints, sizes, u, flags=RECIPE, params=None, left=None):
    """sample_view on the CPU for every (view, sample), driven by the uniforms u [V,B,8].
    -> views [V][B] (dicts with `fragile` and `packed` added)."""
    from peclr_amd.augment import TwoViewAugmenter

    views = []
    for v in range(u.shape[0]):
        row = []
        for i, (j, hw) in enumerate(zip(joints, sizes)):
            j = j.detach().to("cpu", torch.float32).clone()
            if left is not None and left[i]:
                j[:, 0] = int(hw[1]) - j[:, 0]
            aug = TwoViewAugmenter(flags, params, rng=Replay(u[v, i], flags))
            view = aug.sample_view(j, (int(hw[0]), int(hw[1])))
            view["packed"] = aug.pack(view)
            view["fragile"] = is_fragile(j, view)
            row.append(view)
        views.append(row)
    return views


def _near_integer(x):
    return abs(x - round(x)) < FRAGILE_EPS


def is_fragile(j, view):
    """float64 recomputation of what sample_view truncates: the mean x, y of the unrotated joints (the rotation centre) and
    the mean x, y and sqrt(far) * margin of the rotated ones."""
    xy = j[:, :2].double()
    vals = []
    if view["rot"] is not None:
        vals += [float(xy[:, 0].mean()), float(xy[:, 1].mean())]
        hom = j.double().clone()
        hom[:, -1] = 1.0
        xy = (hom @ torch.tensor(view["rot"], dtype=torch.float64).T).float().double()
    mx, my = float(xy[:, 0].mean()), float(xy[:, 1].mean())
    far = float(((xy[:, 1] - int(my)) ** 2 + (xy[:, 0] - int(mx)) ** 2).max())
    vals += [mx, my, math.sqrt(far) * view["crop_margin_scale"]]
    return any(_near_integer(x) for x in vals)
