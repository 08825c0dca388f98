"""What the point-cloud policy's tests share (tests/test_net_cpu.py,
tests/test_gpu_decode.py, tests/test_gpu_net.py, tests/golden/make_net_golden.py):
a seeded state_dict of the reference's model_cls_off_rot.get_model(14, 6, 4),
Inference.predict's decoding restated in f64 numpy for B clouds, and the
network's wiring restated in numpy from given sampling and grouping indices.
"""
import numpy as np

from cloud_reference import group_rows_np, propagate_np

NUM_CLASSES, NUM_INPUT, NUM_OUTPUT = 4, 6, 14
BN_EPS = 1e-5  # torch's BatchNorm default: not part of a state_dict
SA1 = dict(npoint=512, radii=(0.1, 0.2, 0.4), nsamples=(32, 64, 128), widths=[[32, 32, 64], [64, 64, 128], [64, 96, 128]])
SA2 = dict(npoint=128, radii=(0.4, 0.8), nsamples=(64, 128), widths=[[128, 128, 256], [128, 196, 256]])
SA3_WIDTHS, FP3_WIDTHS, FP2_WIDTHS, FP1_WIDTHS = [256, 512, 1024], [256, 256], [256, 128], [128, 128]
START_MASK, END_MASK = 0b1010, 0b1100  # classes 1 and 3, classes 2 and 3
# The seed of the tests' and the golden's weights.  With random weights most
# seeds label every point of a cloud alike (of seeds 1..12 ten do); 9 gives the
# golden's cloud 457 points of class 2 and 143 of class 3, so both point sets
# are populated and differ, with a smallest class margin of 1.9e-4.
STATE_SEED = 9


# ------------------------------------------------------------ the weights
def seeded_state(seed):
    """The state_dict of get_model(14, 6, 4) as key -> array, from
    np.random.default_rng(seed): conv weights normal / sqrt(c_in) in the
    reference's shapes ([o, i, 1, 1] for the set abstractions' Conv2d, [o, i, 1]
    for Conv1d), biases normal * 0.1, batch norms with var in 0.5..2, gamma in
    0.5..1.5, mean and beta non-zero; f32 throughout, and each batch norm's
    num_batches_tracked (i64 0), which load_state_dict asks for."""
    rng = np.random.default_rng(seed)
    f, state = np.float32, {}

    def conv(key, c_out, c_in, tail):
        state[f"{key}.weight"] = (rng.normal(size=(c_out, c_in) + tail) / np.sqrt(c_in)).astype(f)
        state[f"{key}.bias"] = (rng.normal(size=c_out) * 0.1).astype(f)

    def bn(key, c):
        state[f"{key}.weight"] = rng.uniform(0.5, 1.5, c).astype(f)
        state[f"{key}.bias"] = (rng.normal(size=c) * 0.3).astype(f)
        state[f"{key}.running_mean"] = (rng.normal(size=c) * 0.5).astype(f)
        state[f"{key}.running_var"] = rng.uniform(0.5, 2.0, c).astype(f)
        state[f"{key}.num_batches_tracked"] = np.array(0, np.int64)

    def chain(convs, bns, c_in, widths, tail):
        for j, c_out in enumerate(widths):
            conv(f"{convs}.{j}", c_out, c_in, tail)
            bn(f"{bns}.{j}", c_out)
            c_in = c_out

    c_in = NUM_INPUT
    for name, sa in (("sa1", SA1), ("sa2", SA2)):
        for i, widths in enumerate(sa["widths"]):
            chain(f"{name}.conv_blocks.{i}", f"{name}.bn_blocks.{i}", c_in + 3, widths, (1, 1))
        c_in = sum(w[-1] for w in sa["widths"])
    w1, w2 = (sum(w[-1] for w in sa["widths"]) for sa in (SA1, SA2))
    chain("sa3.mlp_convs", "sa3.mlp_bns", w2 + 3, SA3_WIDTHS, (1, 1))
    chain("fp3.mlp_convs", "fp3.mlp_bns", w2 + SA3_WIDTHS[-1], FP3_WIDTHS, (1,))
    chain("fp2.mlp_convs", "fp2.mlp_bns", w1 + FP3_WIDTHS[-1], FP2_WIDTHS, (1,))
    chain("fp1.mlp_convs", "fp1.mlp_bns", 3 + NUM_INPUT + FP2_WIDTHS[-1], FP1_WIDTHS, (1,))
    conv("conv1", 128, FP1_WIDTHS[-1], (1,))
    bn("bn1", 128)
    conv("conv2", NUM_CLASSES + NUM_OUTPUT, 128, (1,))
    return state


# ------------------------------------------------------------- the decode
def euler_xyz_deg(q):
    """scipy's Rotation.from_quat(q).as_euler('xyz', degrees=True) in closed
    form, f64: q [..., 4] xyzw of unit norm -> [..., 3]."""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    with np.errstate(invalid="ignore"):
        roll = np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y))
        pitch = np.arcsin(np.clip(2 * (w * y - z * x), -1, 1))
        yaw = np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))
    return np.degrees(np.stack([roll, pitch, yaw], -1))


def decode_np(head, xyz, nc, centroid=None, scale=None, masks=(START_MASK, END_MASK)):
    """Inference.predict's lines 68-107 in f64 numpy for B clouds, the argmax
    taken on the logits (np.argmax: the lowest index among equal values).
    head [B, N, >= nc + 14], xyz [B, N, 3]; centroid [B, 3] and scale [B] or
    both None; masks the (start, end) class sets as bit masks.  -> a dict of
    labels [B, N] i32, counts [B, 2] i32, first_idx [B, 2] i32 (-1: empty),
    waypoints [B, 2, 3], quats [B, 2, 4], euler_deg [B, 2, 3] f64 (NaN for an
    empty set, where the reference raises)."""
    head, xyz = np.asarray(head, np.float64), np.asarray(xyz, np.float64)
    nb, n = head.shape[:2]
    labels = np.argmax(head[..., :nc], axis=-1).astype(np.int32)
    out = dict(labels=labels, counts=np.zeros((nb, 2), np.int32), first_idx=np.full((nb, 2), -1, np.int32),
               waypoints=np.full((nb, 2, 3), np.nan), quats=np.full((nb, 2, 4), np.nan),
               euler_deg=np.full((nb, 2, 3), np.nan))
    for b in range(nb):
        for k, mask in enumerate(masks):
            idxs = np.where((mask >> labels[b]) & 1)[0]  # ascending, as np.union1d's result
            out["counts"][b, k] = len(idxs)
            if len(idxs) == 0:
                continue
            out["first_idx"][b, k] = idxs[0]
            offsets = head[b, idxs, nc + 3 * k:nc + 3 * k + 3]
            waypt = np.mean(xyz[b, idxs] - offsets, axis=0)
            if centroid is not None:
                waypt = waypt * np.float64(scale[b]) + np.asarray(centroid[b], np.float64)
            out["waypoints"][b, k] = waypt
            rot = head[b, idxs[0], nc + 6 + 4 * k:nc + 10 + 4 * k]
            with np.errstate(invalid="ignore", divide="ignore"):
                out["quats"][b, k] = rot * (1 / np.sqrt(np.sum(rot * rot)))
            out["euler_deg"][b, k] = euler_xyz_deg(out["quats"][b, k])
    return out


# ------------------------------------------------------------ the network
def fold_np(state, conv, bn, dtype):
    """conv (+ bn at inference) as (W [o, i], b [o]) in `dtype`: f32 is
    pandasim.fold_batchnorm (what CloudSegNet uploads), f64 the same fold left
    unrounded, the reference's own layer in exact arithmetic."""
    w = np.asarray(state[f"{conv}.weight"], np.float64)
    w, b = w.reshape(w.shape[:2]), np.asarray(state[f"{conv}.bias"], np.float64)
    if bn is None:
        return w.astype(dtype), b.astype(dtype)
    gamma, beta, mean, var = (np.asarray(state[f"{bn}.{n}"], np.float64)
                              for n in ("weight", "bias", "running_mean", "running_var"))
    if dtype == np.float32:
        from pandasim import fold_batchnorm

        return fold_batchnorm(w, b, gamma, beta, mean, var, BN_EPS)
    s = gamma / np.sqrt(var + BN_EPS)
    return w * s[:, None], (b - mean) * s + beta


def chain_np(state, convs, bns, dtype):
    layers, j = [], 0
    while f"{convs}.{j}.weight" in state:
        layers.append(fold_np(state, f"{convs}.{j}", f"{bns}.{j}", dtype))
        j += 1
    return layers


def mlp_plain(x, layers, last_relu=True):
    """[..., C0] -> [..., C_n] in x's dtype: x @ W.T + b and ReLU per layer
    (plain numpy matmul, no fmaf chain)."""
    for k, (w, b) in enumerate(layers):
        x = x @ w.T + b
        if last_relu or k < len(layers) - 1:
            x = np.maximum(x, 0)
    return x


def propagate_any(xyz1, xyz2, points2, points1, dtype):
    """PointNetFeaturePropagation's tensor before its layers, [B, N, D1 + D2]:
    the kernels' f32 arithmetic (cloud_reference.propagate_np) with f32, the
    same steps in f64 otherwise."""
    if dtype == np.float32:
        return propagate_np(xyz1, xyz2, points2, points1)[0]
    if xyz2.shape[1] == 1:
        interp = np.repeat(points2, xyz1.shape[1], axis=1)
    else:
        d = xyz1[:, :, None, :] - xyz2[:, None, :, :]
        d2 = (d ** 2).sum(-1)
        idx = np.argsort(d2, axis=-1, kind="stable")[..., :3]
        w = 1.0 / (np.take_along_axis(d2, idx, axis=-1) + 1e-8)
        w = w / w.sum(-1, keepdims=True)
        interp = np.stack([(points2[b][idx[b]] * w[b][..., None]).sum(1) for b in range(xyz1.shape[0])])
    return np.concatenate([points1, interp], -1)


def segnet_np(state, xyz, colors, idx, dtype=np.float64):
    """get_model.forward at inference, restated (DESIGN.md §11.6's wiring), on
    given indices: xyz [B, N, 3] the normalised cloud and colors [B, N, 3]
    (f32 values), idx a dict of fps1 [B, 512], group1 (three [B, 512, K]),
    fps2 [B, 128] (into the 512 centres), group2 (two [B, 128, K]); dtype
    np.float64 or np.float32 selects the arithmetic.  -> head [B, N, 18]."""
    x = np.asarray(xyz, dtype)
    l0 = np.concatenate([x, np.asarray(colors, dtype)], -1)
    nb = x.shape[0]
    take = lambda a, i: np.stack([a[b][i[b]] for b in range(nb)])  # noqa: E731

    def msg(name, pts, feats, fps, groups):
        outs = []
        for i, gi in enumerate(groups):
            rows = group_rows_np(pts, feats, fps, gi, dtype)
            y = mlp_plain(rows, chain_np(state, f"{name}.conv_blocks.{i}", f"{name}.bn_blocks.{i}", dtype))
            outs.append(y.max(axis=2))
        return np.concatenate(outs, -1)

    l1 = msg("sa1", x, l0, idx["fps1"], idx["group1"])
    x1 = take(x, idx["fps1"])
    l2 = msg("sa2", x1, l1, idx["fps2"], idx["group2"])
    x2 = take(x1, idx["fps2"])
    l3 = mlp_plain(np.concatenate([x2, l2], -1), chain_np(state, "sa3.mlp_convs", "sa3.mlp_bns", dtype))
    l3 = l3.max(axis=1, keepdims=True)  # group_all: xyz first, one row per cloud
    origin = np.zeros((nb, 1, 3), dtype)
    l2 = mlp_plain(propagate_any(x2, origin, l3, l2, dtype), chain_np(state, "fp3.mlp_convs", "fp3.mlp_bns", dtype))
    l1 = mlp_plain(propagate_any(x1, x2, l2, l1, dtype), chain_np(state, "fp2.mlp_convs", "fp2.mlp_bns", dtype))
    l0 = mlp_plain(propagate_any(x, x1, l1, np.concatenate([x, l0], -1), dtype),
                   chain_np(state, "fp1.mlp_convs", "fp1.mlp_bns", dtype))
    head = [fold_np(state, "conv1", "bn1", dtype), fold_np(state, "conv2", None, dtype)]
    out = mlp_plain(l0, head, last_relu=False)
    assert out.dtype == dtype
    return out
