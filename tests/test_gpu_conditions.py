"""GPU suite for the condition records (buctd_amd/dataset/conditions.py over buctd_pose_boxes / buctd_match_boxes /
buctd_group_max_iou / buctd_group_near_list in csrc/conditions.hip) against the restatement
tests/helpers/condition_ref.py on the seeded sets of tests/helpers/condition_cases.py (K = 17 and K = 5; what they hold
is listed there and checked in tests/test_conditions.py).

Condition on the inputs, asserted on the restatement's values alone: per annotation any two candidates' IoUs are
bit-equal or more than 1e-9 apart, and so are the train overlaps among themselves and against 0 and 1.  Under it every
output is exactly equal to the restatement: boxes, matched, best_iou, cond_kpts, cond_max_iou in both forms, the near
lists, the status words, center / scale as float32 - the kernels run the same fp64 operations in the same order."""
import numpy as np
import pytest
import torch

from tests.helpers import condition_cases as cases
from tests.helpers import condition_ref as ref

pytestmark = pytest.mark.gpu
KS = [17, 5]
EINVAL = -1


def _source(K, dev, gt=True):
    from buctd_amd.dataset.conditions import ConditionSource
    return ConditionSource(cases.cfg(K), cases.case(K)['gt'] if gt else None, device=dev)


def _conditions(r):
    for row in r['rows']:
        assert cases.separated(row['ious']), row
    for ious in r['test_ious']:
        for per_pose in ious:
            assert cases.separated(per_pose)
    for overlaps in r['overlaps'].values():
        assert cases.separated(overlaps, points=(0.0, 1.0))


def _same_record(got, want, fields):
    assert list(got) == list(want)
    for k in fields:
        a, b = got[k], want[k]
        if isinstance(b, dict):
            assert list(a) == list(b), k
            for key in b:
                assert np.array_equal(a[key], b[key]), (k, key)
        elif isinstance(b, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
        elif isinstance(b, list):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), k
        else:
            assert a == b, (k, a, b)


def _pose_boxes(dev, poses, form, mask=None, margin=0.0):
    from buctd_amd import _C
    p = torch.as_tensor(np.ascontiguousarray(poses, dtype=np.float64)).to(dev)
    m = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, dtype=np.int32)).to(dev)
    boxes = torch.full((p.shape[0], 4), -7.0, dtype=torch.float64, device=dev)
    status = torch.full((p.shape[0],), -7, dtype=torch.int32, device=dev)
    _C.check(_C.lib().buctd_pose_boxes(_C.ptr(p), p.shape[0], p.shape[1], form, _C.ptr(m), margin, _C.ptr(boxes),
                                       _C.ptr(status), _C.stream_ptr()), "pose_boxes")
    return boxes.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("K", KS)
def test_pose_boxes_equal_the_restatement_in_both_forms(dev, K):
    c, r = cases.case(K), cases.reference(K)
    # non-zero form: every BU pose and the pose without a non-zero x
    poses = np.concatenate([np.array(b['preds'], dtype=np.float64) for b in c['bu_results']] + [cases.bad_pose(K)[None]])
    boxes, status = _pose_boxes(dev, poses, 1, margin=cases.MARGIN)
    want = [b for image in r['test_boxes'] for b in image] + [None]
    assert status.tolist() == [0 if b is not None else 1 for b in want] and status[-1] == 1
    assert np.array_equal(boxes, np.array([b if b is not None else [0.0] * 4 for b in want]))
    # all-points form: the annotations through their mask, the results without one
    kp = np.array([a['keypoints'] for a in c['gt']['annotations']], dtype=np.float64).reshape(-1, K, 3)
    boxes, status = _pose_boxes(dev, kp, 0, mask=(kp[:, :, 0] != 0) & (kp[:, :, 1] != 0))
    assert status.tolist() == [w['status'] for w in r['rows']]
    for got, w in zip(boxes, r['rows']):
        if w['gt_box'] is not None:
            assert np.array_equal(got, w['gt_box'])
    pred = np.array([x['keypoints'] for x in c['results']], dtype=np.float64).reshape(-1, K, 3)
    boxes, status = _pose_boxes(dev, pred, 0)
    assert not status.any() and np.array_equal(boxes, ref.corner_boxes(pred[:, :, :2])) and (boxes == 0).any()


@pytest.mark.parametrize("K", KS)
def test_match_and_annotate_equal_the_restated_script(dev, K):
    c, r = cases.case(K), cases.reference(K)
    _conditions(r)
    src = _source(K, dev)
    m = src.match(c['results'], cases.MODEL_KEY)
    assert list(src.gt_ids) == [a['id'] for a in c['gt']['annotations']] and m['model_key'] == cases.MODEL_KEY
    assert m['matched'].tolist() == [w['matched'] for w in r['rows']]
    assert m['best_iou'].dtype == np.float64 and m['best_iou'].tolist() == [w['best_iou'] for w in r['rows']]
    assert m['status'].tolist() == [w['status'] for w in r['rows']]
    assert m['cond_kpts'].dtype == np.float64
    assert np.array_equal(m['cond_kpts'], np.array([w['flat'] for w in r['rows']], dtype=np.float64).reshape(-1, K, 3))
    out = src.annotate({cases.MODEL_KEY: c['results']})
    assert out == r['annotated'] and out is not c['gt']
    assert all(a['cond_kpts'] == {} for a in c['gt']['annotations'])           # the input is left as it was


@pytest.mark.parametrize("K", KS)
def test_test_records_equal_the_restated_loader(dev, K):
    c, r = cases.case(K), cases.reference(K)
    _conditions(r)
    got = _source(K, dev, gt=False).test_records(c['bu_results'])
    assert len(got) == len(r['test_db'])
    for a, b in zip(got, r['test_db']):
        _same_record(a, b, list(b))
        assert a['center'].dtype == np.float32 and a['scale'].dtype == np.float32
    bad = [dict(c['bu_results'][0], preds=[cases.bad_pose(K).tolist()], scores=[0.9])]
    with pytest.raises(ValueError, match="no non-zero x"):
        _source(K, dev, gt=False).test_records(bad)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("model_key", [None, cases.MODEL_KEY])
def test_train_records_equal_the_restated_loader(dev, K, model_key):
    from buctd_amd.dataset.conditions import ConditionSource
    r = cases.reference(K)
    _conditions(r)
    aspect = cases.CROP[0] * 1.0 / cases.CROP[1]
    want, _ = ref.train_records(r['annotated'], K, aspect, cases.SCALE_THRE, image_dir=cases.IMAGE_DIR, model_key=model_key)
    got = ConditionSource(cases.cfg(K), r['annotated'], device=dev).train_records(image_dir=cases.IMAGE_DIR,
                                                                                 model_key=model_key)
    assert len(got) == len(want) > 300
    for a, b in zip(got, want):
        _same_record(a, b, list(b))
    assert {t['overlap_status'] for t in got} == {0, 2}
    assert any(len(t['near_joints']) == 0 for t in got) and max(len(t['near_joints']) for t in got) > 4


def test_records_render_the_same_input_as_the_restatements(dev):
    """test_records() through an eval-mode DeviceSamplePipeline at 96 x 64: the same input tensor, byte for byte."""
    import refine_cases
    K = 17
    c, r = cases.case(K), cases.reference(K)
    small = tuple(f"{cases.IMAGE_DIR}/{i:06d}.jpg" for i in cases.SMALL_IMAGES)
    rng = np.random.RandomState(5)
    images = {p: torch.from_numpy(rng.randint(0, 256, (300, 400, 3)).astype(np.uint8)).to(dev) for p in small}
    pick = lambda db: [dict(t, image=images[t['image']]) for t in db if t['image'] in small]
    got, want = pick(_source(K, dev, gt=False).test_records(c['bu_results'])), pick(r['test_db'])
    assert len(got) == len(want) >= 10
    pipe = refine_cases.pipe_for(K)
    x_got, x_want = pipe(got)[0], pipe(want)[0]
    assert x_got.shape == (len(got), x_got.shape[1], 96, 64) and x_got.dtype == x_want.dtype
    assert x_got.cpu().numpy().tobytes() == x_want.cpu().numpy().tobytes()


def test_two_runs_are_bit_identical(dev):
    from buctd_amd.dataset.conditions import ConditionSource
    c, r = cases.case(17), cases.reference(17)
    runs = []
    for _ in range(2):
        src = _source(17, dev)
        m = src.match(c['results'])
        test = src.test_records(c['bu_results'])
        train = ConditionSource(cases.cfg(17), r['annotated'], device=dev).train_records()
        runs.append((m, test, train))
    (m0, t0, r0), (m1, t1, r1) = runs
    for k in ('cond_kpts', 'matched', 'best_iou', 'status'):
        assert m0[k].tobytes() == m1[k].tobytes(), k
    for a, b in zip(t0, t1):
        assert a['center'].tobytes() == b['center'].tobytes() and a['scale'].tobytes() == b['scale'].tobytes()
        assert np.float64(a['cond_max_iou']).tobytes() == np.float64(b['cond_max_iou']).tobytes()
    for a, b in zip(r0, r1):
        assert np.float64(a['cond_max_iou']).tobytes() == np.float64(b['cond_max_iou']).tobytes()
        assert [x.tobytes() for x in a['near_joints']] == [x.tobytes() for x in b['near_joints']]


def test_c_abi_refusals_come_before_any_launch(dev):
    from buctd_amd import _C
    lib, st, P = _C.lib(), _C.stream_ptr(), _C.ptr
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
    f64 = lambda n, v=-7.0: torch.full((n,), v, dtype=torch.float64, device=dev)
    poses, boxes, status = f64(2 * 5 * 3, 1.0), f64(8), i32(-7, -7)
    assert lib.buctd_pose_boxes(P(poses), 2, 0, 0, None, 0.0, P(boxes), P(status), st) == EINVAL
    assert b"K < 1" in lib.buctd_last_error()
    assert lib.buctd_pose_boxes(P(poses), -1, 5, 0, None, 0.0, P(boxes), P(status), st) == EINVAL
    assert lib.buctd_pose_boxes(P(poses), 2, 5, 2, None, 0.0, P(boxes), P(status), st) == EINVAL
    assert b"form" in lib.buctd_last_error()
    for nulled in range(3):
        a = [P(poses), P(boxes), P(status)]
        a[nulled] = None
        assert lib.buctd_pose_boxes(a[0], 2, 5, 1, None, 0.0, a[1], a[2], st) == EINVAL
        assert b"null" in lib.buctd_last_error()
    off, matched, iou, src_boxes = i32(0, 2), i32(-7, -7), f64(2), f64(8, 1.0)
    assert lib.buctd_match_boxes(P(off), P(off), -1, P(src_boxes), None, P(src_boxes), P(matched), P(iou), st) == EINVAL
    for nulled in range(6):
        a = [P(off), P(off), P(src_boxes), P(src_boxes), P(matched), P(iou)]
        a[nulled] = None
        assert lib.buctd_match_boxes(a[0], a[1], 1, a[2], None, a[3], a[4], a[5], st) == EINVAL
        assert b"null" in lib.buctd_last_error()
    max_iou, count, near_off, near = f64(2), i32(-7, -7), torch.tensor([0, 1, 2], device=dev), i32(-7, -7)
    assert lib.buctd_group_max_iou(P(off), -1, P(src_boxes), 1, P(max_iou), P(status), P(count), st) == EINVAL
    assert lib.buctd_group_max_iou(P(off), 1, P(src_boxes), 2, P(max_iou), P(status), P(count), st) == EINVAL
    for nulled in range(4):
        a = [P(off), P(src_boxes), P(max_iou), P(status)]
        a[nulled] = None
        assert lib.buctd_group_max_iou(a[0], 1, a[1], 1, a[2], a[3], P(count), st) == EINVAL
        assert b"null" in lib.buctd_last_error()
    assert lib.buctd_group_near_list(P(off), -1, P(src_boxes), P(near_off), P(near), st) == EINVAL
    for nulled in range(4):
        a = [P(off), P(src_boxes), P(near_off), P(near)]
        a[nulled] = None
        assert lib.buctd_group_near_list(a[0], 1, a[1], a[2], a[3], st) == EINVAL
        assert b"null" in lib.buctd_last_error()
    torch.cuda.synchronize()
    for t in (boxes, iou, max_iou):
        assert bool((t == -7).all())                                           # nothing ran
    for t in (status, matched, count, near):
        assert bool((t == -7).all())
