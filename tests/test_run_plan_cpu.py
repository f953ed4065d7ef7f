"""Which packets exist: the plan of a pass (distributed.pass_plan) against a restatement written
here, and the draws that Input.run and ModelImage._stream make of it, recorded call by call.

The device is tests/oracle_context.py with a recorder on top; the tests pin CALLS (which Output
is built with which seed and first index, which sample_packets / upload / integrate calls
follow), not packets.  Set-up of tests/test_distributed_cpu.py: Na.mercury.bench.input with
endtime 6000 s, 2300 packets in Outputs of 500."""
import contextlib
import inspect
import io
import os

import numpy as np
import pytest

from nexoclom_amd import Input, ModelImage
from nexoclom_amd.Output import Output
from oracle import np_oracle as O
from tests.oracle_context import OracleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUT = os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input')
PARAMS = {'quantity': 'radiance', 'dims': '64,64', 'width': '8,8'}
TOTAL, SIZE, SEED = 2300, 500, 77
PASSES = 5                                # ceil(2300 / 500): the last Output overshoots
KINDS = {'host': dict(sampler='numpy'), 'philox': dict(sampler='device'),
         'pcg64': dict(sampler='device', generator='pcg64')}


def make_inputs():
    inputs = Input(INPUT)
    inputs.options.endtime = type(inputs.options.endtime)(6000., 's')
    return inputs


# ---- 1. the plan of a pass ---------------------------------------------------------------------
def restated_pass(have, want, chunk, made, drawn):
    """The one-rank plan from the rules of Input.run's docstring, as tuples (number within the
    pass, number within the call, size, first_index), and the number of Outputs."""
    todo = want - have
    size = min(todo, chunk)
    passes = -(-todo // size)
    return [(j, made + j, size, drawn + size*j) for j in range(passes)], passes, size


@pytest.mark.parametrize('have,want', [(have, want) for have in (0, 300)
                                       for want in (1, 500, 2300, 2500) if have < want])
@pytest.mark.parametrize('chunk', [500, 2300, 10**6])
def test_pass_plan_against_its_restatement(have, want, chunk):
    """(have = 300, want = 1 is no case: Input.run plans a pass only while have < want.)"""
    from nexoclom_amd.distributed import pass_plan, shard_range
    for made, drawn in ((0, have), (3, have + 1234)):
        whole, passes, size = restated_pass(have, want, chunk, made, drawn)
        assert size*passes >= want - have > size*(passes - 1)
        for world in (1, 2, 3, 8):
            joined = []
            for rank in range(world):
                plan = pass_plan(have, want, chunk, made, drawn, rank, world)
                assert (plan.passes, plan.size) == (passes, size)
                # what the next pass starts from does not depend on the rank
                assert (plan.made, plan.drawn) == (made + passes, drawn + size*passes)
                lo, hi = shard_range(passes, rank, world)
                assert [tuple(entry) for entry in plan.outputs] == whole[lo:hi]
                for entry in plan.outputs:
                    assert entry.call_number == made + entry.number
                    assert entry.size == size
                    assert entry.first_index == drawn + size*entry.number
                joined += [tuple(entry) for entry in plan.outputs]
            assert joined == whole


def test_pass_plan_of_five_outputs_on_eight_ranks_leaves_three_ranks_empty():
    from nexoclom_amd.distributed import pass_plan
    plans = [pass_plan(0, TOTAL, SIZE, 0, 0, rank, 8) for rank in range(8)]
    assert [len(plan.outputs) for plan in plans] == [1]*5 + [0]*3
    assert all(plan.passes == PASSES and plan.size == SIZE for plan in plans)
    assert [plan.outputs[0].first_index for plan in plans[:5]] == [0, 500, 1000, 1500, 2000]


# ---- the recorder ------------------------------------------------------------------------------
class Recorder(OracleContext):
    """OracleContext that logs what is asked of it.  It draws Philox only: ``pcg64`` is logged
    and ignored, ``piece=(offset, whole)`` writes into that slice of a set of ``whole`` packets."""

    def __init__(self, free=1 << 40):
        super().__init__()
        self.events, self.free = [], free

    def mem_info(self):
        return self.free, 1 << 40

    def sample_packets(self, n, seed, first_index=0, download=False, pcg64=None, piece=None,
                       **src):
        self.events.append(('sample', dict(n=int(n), seed=seed, first_index=int(first_index),
                                           pcg64=pcg64, piece=piece)))
        states = np.ascontiguousarray(
            O.sample_x0_philox(int(n), int(seed), int(first_index), **src).T)
        if piece is None:
            self._soa = states
        else:
            offset, whole = piece
            if self._soa is None or self._soa.shape[1] != whole or offset == 0:
                self._soa = np.zeros((8, whole))
            self._soa[:, offset:offset + n] = states
        self.n_packets = self._soa.shape[1]
        return states.copy() if download else None

    def upload_soa(self, soa):
        self.events.append(('upload', np.shape(soa)[1]))
        super().upload_soa(soa)

    def integrate_const(self, *args, **kwargs):
        self.events.append(('integrate', self.n_packets, self._first))
        return super().integrate_const(*args, **kwargs)

    def integrate_const_rows(self, *args, **kwargs):
        self.events.append(('integrate', self.n_packets, self._first))
        return super().integrate_const_rows(*args, **kwargs)

    def of(self, kind):
        return [event[1:] if len(event) > 2 else event[1] for event in self.events
                if event[0] == kind]


RECORDED = ('seed', 'sampler', 'generator', 'first_index', 'window', 'presampled',
            'materialize_x0')


@pytest.fixture
def built(monkeypatch):
    """Every Output construction (the host sampler's happen on worker threads, in any order):
    the record is also left on the Output, so the catalogue tells the order of the run."""
    records, init = [], Output.__init__
    signature = inspect.signature(init)

    def spy(self, *args, **kwargs):
        bound = signature.bind(self, *args, **kwargs)
        bound.apply_defaults()
        given = bound.arguments
        self._record = dict(size=int(given['npackets']), **{key: given[key] for key in RECORDED})
        records.append(self._record)
        init(self, *args, **kwargs)
    monkeypatch.setattr(Output, '__init__', spy)
    return records


def record(size, seed, sampler='numpy', generator='philox', first_index=0, window=None,
           presampled=False, materialize_x0=True):
    return dict(size=size, seed=seed, sampler=sampler, generator=generator,
                first_index=first_index, window=window, presampled=presampled,
                materialize_x0=materialize_x0)


# ---- 2. Input.run ------------------------------------------------------------------------------
def expected_outputs(kind, batch, seed=SEED, made=0, drawn=0, count=PASSES):
    if kind == 'host':
        return [record(SIZE, seed + made + j) for j in range(count)]
    own = kind == 'pcg64'
    return [record(SIZE, seed + made + j if own else seed, 'device', 'pcg64' if own else 'philox',
                   first_index=drawn + SIZE*j, presampled=batch, materialize_x0=not batch)
            for j in range(count)]


def check_run(kind, batch, ctx, inputs, outputs, launches):
    """``outputs``: the records of the Outputs this call made, in catalogue order; ``launches``:
    the lists of Outputs handed to Output.integrate_batch, in order."""
    counts = [n//SIZE for n, _ in ctx.of('integrate')]
    assert [n for n, _ in ctx.of('integrate')] == [SIZE*c for c in counts]
    assert sum(counts) == len(outputs)
    limit = inputs._group_limit(SIZE, ctx) if batch else 1
    assert all(1 <= c <= limit for c in counts), (counts, limit)
    # the launches partition the Outputs of the run in order
    edges = np.concatenate([[0], np.cumsum(counts)])
    groups = [outputs[a:b] for a, b in zip(edges, edges[1:])]
    if batch:
        assert [[out._record for out in group] for group in launches] == groups
    else:
        assert launches == []
    leads = [group[0]['first_index'] for group in groups]
    assert [at for _, at in ctx.of('integrate')] == leads      # (the host sampler's: all 0)
    if kind == 'host':
        assert ctx.of('sample') == []
        assert ctx.of('upload') == [SIZE*c for c in counts]
    else:
        assert ctx.of('upload') == []
        want = []
        for group, lead in zip(groups, leads):
            if kind == 'philox' and batch:
                want.append(dict(n=SIZE*len(group), seed=group[0]['seed'], first_index=lead,
                                 pcg64=None, piece=None))
            elif kind == 'philox':
                want.append(dict(n=SIZE, seed=group[0]['seed'], first_index=lead, pcg64=None,
                                 piece=None))
            else:
                # every Output of a group follows its own stream into its piece of the set; all
                # are numbered from the group's first index
                want += [dict(n=SIZE, seed=out['seed'], first_index=lead, pcg64=(SIZE, 0),
                              piece=(g*SIZE, SIZE*len(group)) if batch else None)
                         for g, out in enumerate(group)]
        assert ctx.of('sample') == want


@pytest.fixture
def launches(monkeypatch):
    seen, batch = [], Output.integrate_batch.__func__

    def spy(cls, outputs, ctx, save=True):
        seen.append(list(outputs))
        return batch(cls, outputs, ctx, save)
    monkeypatch.setattr(Output, 'integrate_batch', classmethod(spy))
    return seen


def run(inputs, ctx, kind, batch, npackets=TOTAL, seed=SEED):
    with contextlib.redirect_stdout(io.StringIO()) as said:
        inputs.run(npackets, packs_per_it=SIZE, seed=seed, context=ctx, batch=batch, **KINDS[kind])
    return said.getvalue()


# a third of the free memory takes two Outputs of 500 packets (201 records of 80/4 bytes + 192)
ROOM_FOR_TWO = 3*2*SIZE*(201*20 + 192) + 5


@pytest.mark.parametrize('batch', [True, False])
@pytest.mark.parametrize('kind', list(KINDS))
def test_the_draws_of_input_run(kind, batch, built, launches):
    inputs, ctx = make_inputs(), Recorder()
    said = run(inputs, ctx, kind, batch)
    made = [out._record for out in inputs._catalogue]
    assert made == expected_outputs(kind, batch)
    assert sorted(built, key=repr) == sorted(made, key=repr)          # and no others
    assert [out.npackets for out in inputs._catalogue] == [SIZE]*PASSES
    check_run(kind, batch, ctx, inputs, made, launches)
    assert f'Will complete {PASSES} iterations of {SIZE} packets.' in said
    # the host pipeline does not announce its iterations one by one
    assert ('Starting iteration #1 of 5' in said) == (not (kind == 'host' and batch))
    assert said.count('Completed iteration #') == len(ctx.of('integrate'))


@pytest.mark.parametrize('kind', list(KINDS))
def test_the_draws_of_input_run_in_launches_of_two(kind, built, launches):
    """HBM for two Outputs a launch: the seeds and first indices go on across the launches."""
    inputs, ctx = make_inputs(), Recorder(free=ROOM_FOR_TWO)
    assert inputs._group_limit(SIZE, ctx) == 2
    run(inputs, ctx, kind, True)
    made = [out._record for out in inputs._catalogue]
    assert made == expected_outputs(kind, True)
    check_run(kind, True, ctx, inputs, made, launches)
    assert len(launches) >= 3
    if kind != 'host':                       # nothing to wait for: every launch is full
        assert [len(group) for group in launches] == [2, 2, 1]


@pytest.mark.parametrize('kind', list(KINDS))
def test_a_second_call_of_input_run_goes_on_where_the_catalogue_ends(kind, built, launches):
    """1000 packets, then up to 2300 (three more Outputs of 500): the second call counts its
    Outputs from 0 again (seed + k), the Philox index space goes on after the 1000 catalogued."""
    inputs = make_inputs()
    run(inputs, Recorder(), kind, True, npackets=1000)
    del launches[:]
    ctx = Recorder()
    run(inputs, ctx, kind, True)
    made = [out._record for out in inputs._catalogue]
    assert made[:2] == expected_outputs(kind, True, count=2)
    assert made[2:] == expected_outputs(kind, True, drawn=1000, count=3)
    check_run(kind, True, ctx, inputs, made[2:], launches)


@pytest.mark.parametrize('kind', ['philox', 'pcg64'])
def test_a_group_split_in_halves_is_drawn_again_from_the_same_seeds(kind, built):
    """Rows for 1000 packets only: the launch of five Outputs is split (2, 3), the three again
    (1, 2), and every attempt draws its Outputs from their own seeds and its lead's index."""
    from nexoclom_amd import hip_api

    class Tight(Recorder):
        def integrate_const_rows(self, *args, **kwargs):
            if self.n_packets > 1000:
                self.events.append(('refused', self.n_packets))
                raise hip_api.HipError('no room for the rows of this launch group',
                                       hip_api.NXC_ERR_NOMEM)
            return super().integrate_const_rows(*args, **kwargs)
    inputs, ctx = make_inputs(), Tight()
    run(inputs, ctx, kind, True)
    made = [out._record for out in inputs._catalogue]
    assert made == expected_outputs(kind, True)
    assert ctx.of('refused') == [2500, 1500]
    assert ctx.of('integrate') == [(1000, 0), (500, 1000), (1000, 1500)]
    attempts = [made, made[:2], made[2:], made[2:3], made[3:]]
    if kind == 'philox':
        want = [dict(n=SIZE*len(group), seed=SEED, first_index=group[0]['first_index'],
                     pcg64=None, piece=None) for group in attempts]
    else:
        want = [dict(n=SIZE, seed=out['seed'], first_index=group[0]['first_index'],
                     pcg64=(SIZE, 0), piece=(g*SIZE, SIZE*len(group)))
                for group in attempts for g, out in enumerate(group)]
    assert ctx.of('sample') == want


def test_an_unseeded_device_run_has_one_key(built, launches):
    inputs, ctx = make_inputs(), Recorder()
    run(inputs, ctx, 'philox', True, seed=None)
    made = [out._record for out in inputs._catalogue]
    key = made[0]['seed']
    assert isinstance(key, int) and 0 <= key < 2**64
    assert made == expected_outputs('philox', True, seed=key)
    check_run('philox', True, ctx, inputs, made, launches)
    assert {call['seed'] for call in ctx.of('sample')} == {key}


# ---- 3. ModelImage._stream ---------------------------------------------------------------------
def stream(kind, shard, seed=SEED):
    ctx = Recorder()
    with contextlib.redirect_stdout(io.StringIO()):
        image = ModelImage(make_inputs(), PARAMS, npackets=TOTAL, packs_per_it=SIZE, seed=seed,
                           context=ctx, shard=shard, finalize=False, **KINDS[kind])
    return ctx, image


def pieces(lo, hi):
    """(k, chunk start, chunk length, a, b) of the chunk grid of 2300 in 500s over [lo, hi)."""
    out = []
    for k in range(PASSES):
        c0, clen = SIZE*k, min(SIZE, TOTAL - SIZE*k)
        a, b = max(lo, c0), min(hi, c0 + clen)
        if b > a:
            out.append((k, c0, clen, a, b))
    return out


def check_stream(kind, ctx, image, built, lo, hi, windowed=True):
    plan = pieces(lo, hi)
    assert ctx.of('integrate') == [(b - a, a) for _, _, _, a, b in plan]
    assert image.seed == SEED and image.npackets == hi - lo
    assert image.totalsource == (hi - lo)*201
    assert image.counters['particle_steps'] > 0
    if kind == 'host':
        # one Output a chunk from seed + k; a cut chunk draws only its rows when it can
        want = []
        for k, c0, clen, a, b in plan:
            cut = windowed and (a - c0, b - c0) != (0, clen)
            want.append(record(clen, SEED + k, window=(clen, a - c0, b - c0) if cut else None))
        assert sorted(built, key=repr) == sorted(want, key=repr)
        assert ctx.of('sample') == []
        assert ctx.of('upload') == [b - a for _, _, _, a, b in plan]
        return
    assert ctx.of('upload') == []
    k, c0, clen, a, b = plan[0]            # the first chunk's Output describes the source
    if kind == 'philox':
        assert built == [record(b - a, SEED, 'device', first_index=a, materialize_x0=False)]
        assert ctx.of('sample') == [dict(n=b - a, seed=SEED, first_index=a, pcg64=None, piece=None)
                                    for _, _, _, a, b in plan]
    else:
        assert built == [record(clen, SEED + k, 'device', 'pcg64', first_index=a,
                                window=(clen, a - c0, b - c0), materialize_x0=False)]
        assert ctx.of('sample') == [dict(n=b - a, seed=SEED + k, first_index=a,
                                         pcg64=(clen, a - c0), piece=None)
                                    for k, c0, clen, a, b in plan]


@pytest.mark.parametrize('shard', [None, (700, 1900)])
@pytest.mark.parametrize('kind', list(KINDS))
def test_the_draws_of_the_streaming_image(kind, shard, built):
    ctx, image = stream(kind, shard)
    lo, hi = shard or (0, TOTAL)
    assert len(pieces(lo, hi)) == (5 if shard is None else 3)
    check_stream(kind, ctx, image, built, lo, hi)
    assert image.packet_image.sum() > 100


def test_a_cut_chunk_that_cannot_be_windowed_is_drawn_whole_and_sliced(built, monkeypatch):
    from nexoclom_amd.source_distribution import WindowGenerator
    monkeypatch.setattr(WindowGenerator, 'windowable', staticmethod(lambda inputs: False))
    ctx, image = stream('host', (700, 1900))
    check_stream('host', ctx, image, built, 700, 1900, windowed=False)


@pytest.mark.parametrize('kind', list(KINDS))
def test_an_empty_shard_of_the_streaming_image(kind, built):
    """Nothing is drawn or integrated; a host Output of no packets sets the (zero) image up."""
    ctx, image = stream(kind, (700, 700))
    assert built == [record(0, SEED)]
    assert ctx.events == []
    assert image.seed == SEED and image.npackets == 0 and image.totalsource == 0
    assert image.counters == {}
    assert image.image.shape == (64, 64) and not image.image.any()
    assert not image.packet_image.any()
