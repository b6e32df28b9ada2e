"""CPU: the route table of the optimiser update.  Every combination of engine, optimiser, loss scaler, group, regularisation,
schedule and averaging takes one eager `step`, `run_plan(1, 0)` and (TrainEngine) `run_plan(1, -1)` under the recorder of
tests/test_engine_update_host.py, and the launches — every entry point, its scalars, its pointers by the engine tensor they point
into, in order — must be the ones tests/golden/g14_update_routes.json holds, together with `_hparams()`, `_counts_on_device()`,
`_graphable()`, `_native_loop_ok()` and the step counts afterwards.  A combination that the constructor or a setter refuses is
held as the refusal's message.

The fixture is a recording of the commit it names (`parent`), made by `python tests/test_update_routes_host.py --record` in a
checkout of that commit with this file copied in.  It is never regenerated from a later tree: a launch that differs from it is a
change of behaviour.  It holds the distinct routes once — a route is a sequence's entry points by name, the readable table — and
per engine kind a row `optimiser|scaler|group|regularisation` of six cells (schedule none / epoch / step × averaging none / ema):
[route of the step, of the plan step, of the native loop (null: stage 2), digest], or the index of the refusal's message (one index
where the whole row is refused by it).  The digest is the first 10 hex digits of the SHA-256 of the cell's whole record as
compact JSON with sorted keys: every scalar, every pointer name, the state.  A cell that differs is reported with its record.

The recorder here leaves nothing anonymous: the engine tensors the sibling tests do not name are named, the structs are
expanded into their fields, the mean loss the general route scatters into the loss history is recorded, and a pointer into no
known tensor is an error."""
import hashlib
import itertools
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == '__main__':                 # run as a script (--record): the path the suite's conftest.py sets
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'dual-modal-fusion_amd'))

from test_engine_update_host import DQTL, Ptr, Recorder

FIXTURE = os.path.join(HERE, 'golden', 'g14_update_routes.json')
ENGINES = ('late', 'attn', 'late-criterion', 'attn-criterion', 'qua-unit', 'qua-nonunit')
AXES = (('ADAM', 'ADAMW', 'SGD', 'RMSprop'), ('fp32', 'scaler'), ('single', 'collective', 'xgmi'),
        ('none', 'decay', 'clip'), ('none', 'epoch', 'step'), ('none', 'ema'))
REG = {'none': {}, 'decay': dict(weight_decay=0.01), 'clip': dict(clip_grad_norm=0.5)}
TABLE = np.array([[1e-3, 0.9, 0.999, 0.5], [5e-4, 0.85, 0.999, 0.4]], dtype=np.float32)
CRITERION = {'kind': 'ce', 'label_smoothing': 0.1, 'class_weights': np.linspace(0.5, 2.0, 5).tolist()}
B, K = 8, 5
# engine tensors that test_engine_update_host.NAMED leaves out
MORE = ('avg', 'norm', 'norm_hist', 'hp_table', 'hp_row', 'plan_denom', 'denom', 'short_xy', 'short_labels', 'win', 'plan_pack')


def _f32(x):
    return float(np.float32(x))


def _ptr(p):
    return Ptr(p) if p else None


def _anonymous(c):
    return c == '?' or (isinstance(c, tuple) and any(_anonymous(x) for x in c))


class RouteRecorder(Recorder):
    gathered = None                          # the coordinates of the last input_gather (stage 2 stacks an eager batch's itself)

    @staticmethod
    def arg(a):
        from dmf import lib
        obj = getattr(a, '_obj', None)
        if isinstance(obj, lib.HpSchedule):
            return ('sched', _ptr(obj.table), obj.rows, _ptr(obj.row_dev))
        if isinstance(obj, lib.WeightAvg):
            return ('avg', _ptr(obj.avg), obj.kind, _f32(obj.weight), obj.start, obj.reserved)
        if isinstance(obj, lib.CeFused):
            p = obj.params.contents
            return ('ce_fused', (p.kind, _f32(p.label_smoothing), _f32(p.gamma)), _ptr(obj.class_w), _ptr(obj.labels_global),
                    _ptr(obj.denom), obj.ranks, obj.rank, _f32(obj.grad_scale), obj.reserved)
        return Recorder.arg(a)

    def take(self, eng, **extra):
        more = {n: getattr(eng, n) for n in MORE if getattr(eng, n, None) is not None}
        if self.gathered is not None:
            extra = dict(extra, stacked_xy=self.gathered)
        calls = super().take(eng, **more, **extra)
        for c in calls:
            assert not _anonymous(c), 'a pointer into no known tensor: %r' % (c,)
        return calls


class recording:
    """`with recording() as rec`: the library behind dmf.lib, the group's collectives and Tensor.scatter_ record into rec."""

    def __enter__(self):
        import torch.distributed as dist
        from dmf import lib
        self.mp = mp = pytest.MonkeyPatch()
        rec = RouteRecorder(lib._lib)
        mp.setattr(lib, '_lib', rec)
        mp.setattr(lib, '_dev', lambda t, dtype, name: t)
        mp.setattr(lib, '_stream', lambda: None)
        for entry in ('all_reduce', 'all_gather', 'all_gather_into_tensor'):
            mp.setattr(dist, entry, rec.collective(getattr(dist, entry), entry))
        gather, scatter = lib.input_gather, torch.Tensor.scatter_

        def input_gather(*args, **kw):
            rec.gathered = args[3]
            return gather(*args, **kw)

        def scatter_(t, *args, **kw):
            rec.calls.append(('scatter_', Ptr(t.data_ptr())))
            return scatter(t, *args, **kw)
        mp.setattr(lib, 'input_gather', input_gather)
        mp.setattr(torch.Tensor, 'scatter_', scatter_)
        return rec

    def __exit__(self, *exc):
        self.mp.undo()


def _engine(kind, optim, scaler, group, reg):
    from dmf import lib
    from dmf.engine import LossScaler, QuaScene, QuaTrainEngine, Scene, TrainEngine
    from model.gmfnet import Net
    kw = dict(lr=2e-3, process_group=group, scaler=LossScaler('cpu') if scaler else None, optimizer=optim, momentum=0.5, **reg)
    torch.manual_seed(0)
    if kind.startswith('qua'):               # the net of test_engine_update_host
        cfg = {'patch_size': 16, 'Categories_Number': K, 'data_city': 's', 'DATA_DICT': {'s': {'size': [20, 20, 4]}},
               'gmf': {'width': 40, 'single_input': 1}}
        with pytest.MonkeyPatch.context() as mp:
            if kind == 'qua-nonunit':
                mp.setattr(lib, 'unit_supported', lambda shape: False)
            return QuaTrainEngine(Net(cfg), QuaScene([np.zeros((36, 36, 4), np.float32)] * 4, 'cpu'), B, DQTL, **kw)
    cfg = {'patch_size': 5, 'Categories_Number': K, 'data_city': 's', 'DATA_DICT': {'s': {'size': [20, 20, 8]}}, 'scale': 1,
           'aux_bands': 1, 'gmf': {'width': 40, 'hidden': 64, 'pool_sigma': 2.5, 'attention': int(kind.startswith('attn'))},
           'trans': {'embed_dim': 96, 'num_head': 3}}
    scene = Scene(np.zeros((24, 24, 8), np.float32), np.zeros((24, 24, 1), np.float32), 'cpu')
    if kind.endswith('criterion'):
        kw.update(criterion=CRITERION, criterion_in_kernel=kind == 'attn-criterion')
    return TrainEngine(Net(cfg), scene, B, **kw)


def run_cell(kind, cell, rec, group):
    """One cell of the table on the tree under test: {'refusal': message}, or the three launch sequences and the state."""
    from dmf import lib
    optim, scaler, grp, reg, sched, avg = cell
    try:
        eng = _engine(kind, optim, scaler == 'scaler', None if grp == 'single' else group, REG[reg])
        eng._force_collective = grp != 'single'
        if grp == 'xgmi':                    # (the constructor keeps a communicator only for world > 1)
            eng.comm = types.SimpleNamespace(c=lib.XgmiComm(world=1), world=1, capacity=eng.theta.numel(), rewind=lambda n: None)
        if sched != 'none':
            eng.set_schedule(TABLE, sched)
        if avg != 'none':
            eng.set_averaging(avg, 0.99, 4)
    except lib.DmfError as e:
        return {'refusal': str(e)}
    state = {'hparams': list(eng._hparams()), 'counts_on_device': eng._counts_on_device(), 'graphable': eng._graphable()}
    if hasattr(eng, '_native_loop_ok'):
        state['native_loop_ok'] = eng._native_loop_ok()
    rng = np.random.default_rng(0)
    xy = torch.from_numpy(rng.integers(0, 20, (B, 2)).astype(np.int32))
    labels = torch.from_numpy(rng.integers(0, K, B).astype(np.int32))
    out = {}
    rec.calls = []
    eng.step(xy, labels)
    out['step'] = rec.take(eng, xy=xy, labels=labels)
    eng.load_plan(rng.integers(0, 20, (2 * B, 2)).astype(np.int32), rng.integers(0, K, 2 * B).astype(np.int32))
    rec.calls = []
    assert eng.run_plan(1, 0) == 1
    out['plan'] = rec.take(eng)
    if hasattr(eng, '_native_loop_ok'):
        assert eng.run_plan(1, -1) == 1
        out['native'] = rec.take(eng)
    state.update(step_count=eng.step_count, host_cursor=eng.host_cursor)
    return json.loads(json.dumps(dict(out, state=state)))        # (as the fixture holds it: tuples are lists)


def cells():
    return list(itertools.product(*AXES))


COLUMNS = list(itertools.product(*AXES[4:]))          # a row's six cells: schedule x averaging


def summary(record):
    """What the fixture holds of run_cell's record: the refusal's message, or the three routes by name and the digest of all of it."""
    if 'refusal' in record:
        return record['refusal']
    digest = hashlib.sha256(json.dumps(record, sort_keys=True, separators=(',', ':')).encode()).hexdigest()[:10]
    return [[c[0] for c in record[n]] if n in record else None for n in ('step', 'plan', 'native')] + [digest]


def resolve(doc, kind, cell):
    """The fixture's cell as `summary` returns it."""
    row = doc['engines'][kind]['|'.join(cell[:4])]
    at = row if isinstance(row, int) else row[COLUMNS.index(cell[4:])]
    if isinstance(at, int):
        return doc['refusals'][at]
    return [None if i is None else doc['routes'][i] for i in at[:3]] + [at[3]]


@pytest.fixture(scope='module')
def group(tmp_path_factory):
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method='file://%s' % tmp_path_factory.mktemp('pg').joinpath('store'), rank=0, world_size=1)
    yield dist.group.WORLD
    dist.destroy_process_group()


def differing_cells(kind, doc, group):
    """-> ({cell key: its record on this tree} of the cells that differ from the fixture's, the routes that were reached)."""
    wrong, reached = {}, []
    with recording() as rec:
        for cell in cells():
            record = run_cell(kind, cell, rec, group)
            got = summary(record)
            if got != resolve(doc, kind, cell):
                wrong['|'.join(cell)] = record
            reached += [r for r in got[:3] if r is not None] if isinstance(got, list) else []
    return wrong, reached


@pytest.mark.parametrize('kind', ENGINES)
def test_update_routes(kind, group):
    doc = json.load(open(FIXTURE))
    assert sorted(doc['engines'][kind]) == sorted({'|'.join(c[:4]) for c in cells()})
    wrong, reached = differing_cells(kind, doc, group)
    assert not wrong, '%d cells differ from the recorded table: %s; the first one now gives %s' % (
        len(wrong), sorted(wrong)[:12], json.dumps(next(iter(wrong.values())), indent=1))
    # no route of this engine kind's table has dropped out of reach
    used = {i for row in doc['engines'][kind].values() if not isinstance(row, int) for at in row if not isinstance(at, int)
            for i in at[:3] if i is not None}
    assert {doc['routes'].index(r) for r in reached} == used


def test_every_route_and_refusal_of_the_table_belongs_to_a_cell():
    doc = json.load(open(FIXTURE))
    cells_ = [at for t in doc['engines'].values() for row in t.values() for at in ([row] if isinstance(row, int) else row)]
    assert {at for at in cells_ if isinstance(at, int)} == set(range(len(doc['refusals'])))
    assert {i for at in cells_ if not isinstance(at, int) for i in at[:3] if i is not None} == set(range(len(doc['routes'])))


# ------------------------------------------------------------------------------------------------ recording (the parent only)
def _pack(doc, kind, records):
    """{cell: run_cell's record} of one engine kind -> its rows in doc."""
    def at(name, item):
        if item not in doc[name]:
            doc[name].append(item)
        return doc[name].index(item)
    rows = doc['engines'][kind] = {}
    for cell in cells():
        got = summary(records[cell])
        rows.setdefault('|'.join(cell[:4]), []).append(
            at('refusals', got) if isinstance(got, str) else [None if r is None else at('routes', r) for r in got[:3]] + [got[3]])
    for key, row in rows.items():
        if isinstance(row[0], int) and row == [row[0]] * len(COLUMNS):
            rows[key] = row[0]


def _dump(doc, f):
    """JSON, one route, refusal and row per line."""
    line = lambda x: json.dumps(x, separators=(',', ':'))
    f.write('{\n"parent":%s,\n"routes":[\n' % line(doc['parent']) + ',\n'.join(line(x) for x in doc['routes']))
    f.write('\n],\n"refusals":[\n' + ',\n'.join(line(x) for x in doc['refusals']) + '\n],\n"engines":{\n')
    f.write(',\n'.join('%s:{\n' % line(kind) + ',\n'.join('%s:%s' % (line(k), line(row)) for k, row in rows.items()) + '\n}'
                       for kind, rows in doc['engines'].items()))
    f.write('\n}\n}\n')


def record():
    import subprocess
    import tempfile
    import torch.distributed as dist
    parent = subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=HERE, text=True).strip()
    doc = {'parent': parent, 'routes': [], 'refusals': [], 'engines': {}}
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group('gloo', init_method='file://%s' % os.path.join(tmp, 'store'), rank=0, world_size=1)
        with recording() as rec:
            for kind in ENGINES:
                records = {c: run_cell(kind, c, rec, dist.group.WORLD) for c in cells()}
                _pack(doc, kind, records)
                ran = [json.dumps(r[n]) for r in records.values() for n in ('step', 'plan', 'native') if n in r]
                print('%-15s %3d cells, %3d refused, %3d distinct sequences' % (
                    kind, len(records), sum('refusal' in r for r in records.values()), len(set(ran))))
        dist.destroy_process_group()
    with open(FIXTURE, 'w') as f:
        _dump(doc, f)
    json.load(open(FIXTURE))
    print('%s: %d bytes, %d routes, %d refusals, recorded from %s' % (
        FIXTURE, os.path.getsize(FIXTURE), len(doc['routes']), len(doc['refusals']), parent))


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit('usage: python tests/test_update_routes_host.py --record    (in a checkout of the parent commit)')
    record()
