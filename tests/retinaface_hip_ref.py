"""Cases, seeded inputs and the float64 detection flow shared by the RetinaFace HIP-backend tests and tools/make_golden_retinaface_hip.py.

Weights: oracle.make_golden_retinaface.build (the 'resnet50' case's seeded state_dict).  Inputs: its seeded_frames.  The fixture
tests/golden/retinaface_hip_ref.npz holds, per case, the reference module's own forward in float32 (`_loc32`, `_conf32`, `_ldm32`) and in
float64 (`_loc64` ...), and for FLOW_CASE the float64 detection flow's threshold and rows.  Nothing here needs the reference tree.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import make_golden_retinaface as G  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'retinaface_hip_ref.npz')
NET_CASE = G.CASES['resnet50']
# (n, h, w, 3) frames and their seed: the existing fixture's batch (odd at every stride-2 layer: 150x210 -> 75x105 -> 38x53 -> 19x27 -> 10x14 -> 5x7,
# FPN resizes 5 -> 10, 10 -> 19 and 7 -> 14, 14 -> 27), an even case, and a tall odd one
CASES = {'b2_150x210': dict(shape=NET_CASE['shape'], seed=NET_CASE['in_seed']),
         'b1_64x96': dict(shape=(1, 64, 96, 3), seed=52),
         'b1_97x33': dict(shape=(1, 97, 33, 3), seed=53),
         'b2_48x80': dict(shape=(2, 48, 80, 3), seed=74)}
NET_CASES = ('b2_150x210', 'b1_64x96', 'b1_97x33')
# The detection flow's case, chosen on the CPU among seeded small batches: 26 / 32 candidates, 12 / 13 rows after NMS, score gap 1.7e-2 and smallest
# |IoU - nms| 1.1e-3 against 100 e_ref = 1.8e-4.  (The first case has 225 candidates per image and with them a pair 3.9e-5 from the NMS threshold.)
FLOW_CASE = 'b2_48x80'
OUTS = ('loc', 'conf', 'ldm')
MEAN = (104., 117., 123.)
VARIANCE = (0.1, 0.2)
NMS = 0.4
SCORE_BAND = (0.6, 0.9)


def build(cls, **kw):
    return G.build(cls, NET_CASE, **kw)


def case_frames(case):
    c = CASES[case]
    return G.seeded_frames(c['shape'], c['seed'])


def case_input(case):
    """(n,3,h,w) float32: the frames minus the detector's BGR mean."""
    f = torch.from_numpy(case_frames(case).astype(np.float32)).permute(0, 3, 1, 2)
    return (f - torch.tensor(MEAN).view(1, 3, 1, 1)).contiguous()


def golden():
    return np.load(GOLDEN)


def decode64(loc, ldm, priors, w, h, resize=1.0):
    """retinaface_utils.decode / decode_landm and the `* scale / resize` products in float64: (n,4) boxes, (n,10) landmarks in pixels."""
    loc, ldm, p = (np.asarray(a, dtype=np.float64) for a in (loc, ldm, priors))
    centre = p[:, :2] + loc[:, :2] * VARIANCE[0] * p[:, 2:]
    size = p[:, 2:] * np.exp(loc[:, 2:] * VARIANCE[1])
    lo = centre - size / 2
    boxes = np.concatenate((lo, size + lo), axis=1) * np.array([w, h, w, h], dtype=np.float64) / resize
    pts = np.concatenate([p[:, :2] + ldm[:, 2 * k:2 * k + 2] * VARIANCE[0] * p[:, 2:] for k in range(5)], axis=1)
    return boxes, pts * np.array([w, h] * 5, dtype=np.float64) / resize


def iou64(a, b):
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = w * h
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def flow64(loc, conf, ldm, priors, w, h, thr, nms=NMS):
    """The detection flow of one image in float64: rows (k,15) [box, score, landmarks] after the threshold and greedy NMS in descending score
    order (detect_faces sorts first, batched_detect_faces lets NMS order the rows: the same rows in the same order); and the smallest
    |IoU - nms| over every pair of candidates."""
    boxes, pts = decode64(loc, ldm, priors, w, h)
    s = np.asarray(conf, dtype=np.float64)[:, 1]
    idx = np.where(s > thr)[0]
    order = idx[np.argsort(-s[idx], kind='stable')]
    margin = min([abs(iou64(boxes[i], boxes[j]) - nms) for a, i in enumerate(order) for j in order[a + 1:]], default=np.inf)
    keep, alive = [], np.ones(len(order), dtype=bool)
    for a, i in enumerate(order):
        if not alive[a]:
            continue
        keep.append(i)
        for b in range(a + 1, len(order)):
            if alive[b] and iou64(boxes[i], boxes[order[b]]) > nms:
                alive[b] = False
    keep = np.asarray(keep, dtype=np.int64)
    return np.concatenate((boxes[keep], s[keep, None], pts[keep]), axis=1), margin


def pick_threshold(scores):
    """(threshold, gap): the middle of the widest gap between neighbouring float64 scores inside SCORE_BAND, over all images of the case."""
    s = np.sort(np.asarray(scores, dtype=np.float64).reshape(-1))
    s = s[(s >= SCORE_BAND[0]) & (s <= SCORE_BAND[1])]
    assert s.size >= 2, 'fewer than two scores in the band'
    g = np.diff(s)
    k = int(np.argmax(g))
    return float((s[k] + s[k + 1]) / 2), float(g[k])
