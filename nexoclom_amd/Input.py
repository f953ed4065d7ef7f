"""Input: the inputfile-driven front door of a model run.

Drop-in for the reference's initial_state/Input.py:27-272 on the hot path: ``Input(infile)`` turns
the ``section.key = value`` lines of an inputfile into seven section objects (``geometry``,
``surfaceinteraction``, ``forces``, ``spatialdist``, ``speeddist``, ``angulardist``,
``options``); ``run()`` integrates packets chunk by chunk; ``search()`` tells what has been run;
``produce_image()`` builds a ModelImage.  The file grammar is the reference's (Input.py:60-80): a
``;`` -- or, on lines without one, a ``#`` -- starts a comment; a line counts only if it holds
exactly one ``=`` and the left side exactly one ``.``; section and key are case-folded.

The reference catalogues runs in PostgreSQL; here the catalogue is the list of Output objects kept
on the Input (plus optional .npz files under ``savepath``).
"""
import math
import os
import time

from . import input_classes as spec
from .Output import Output
from .distributed import pass_plan, shard_range
from .draws import DrawAhead, Draws

HOST_SAMPLER_THREADS = 8        # Outputs drawn side by side, ahead of the device (16: no faster)

# section name in the file -> (attribute on the Input, class that interprets it)
SECTIONS = (('geometry', spec.Geometry), ('surfaceinteraction', spec.SurfaceInteraction),
            ('forces', spec.Forces), ('spatialdist', spec.SpatialDist),
            ('speeddist', spec.SpeedDist), ('angulardist', spec.AngularDist),
            ('options', spec.Options))


def read_inputfile(path):
    """{section: {key: value text}} of an inputfile; later lines override earlier ones."""
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    table = {}
    with open(path, 'r') as handle:
        for raw in handle:
            mark = ';' if ';' in raw else '#'
            text = raw.split(mark, 1)[0]
            left, eq, right = text.partition('=')
            if not eq or '=' in right:
                continue
            section, dot, key = left.partition('.')
            if not dot or '.' in key:
                continue
            table.setdefault(section.casefold().strip(), {})[key.casefold().strip()] = right.strip()
    return table


class Input:
    def __init__(self, infile, savepath=None):
        self._inputfile, self.savepath = infile, savepath
        self._catalogue = []          # Output objects run with these inputs
        self._fused = []              # fused integrate+image results (ModelImage streaming mode)
        table = read_inputfile(infile)
        for name, cls in SECTIONS:
            setattr(self, name, cls(table.get(name, {})))
        spec.check_map_laws(self.spatialdist, self.speeddist, self.angulardist)

    def _sections(self):
        return [getattr(self, name) for name, _ in SECTIONS]

    def __copy__(self):
        # a copy shares the catalogue (ModelResult copies its inputs) but not the writer thread
        new = type(self).__new__(type(self))
        new.__dict__.update({k: v for k, v in self.__dict__.items()
                             if k not in ('_writer', '_pending')})
        return new

    def __eq__(self, other):
        return isinstance(other, type(self)) and self._sections() == other._sections()

    __hash__ = None

    def __str__(self):
        return '\n'.join(str(section) for section in self._sections())

    __repr__ = __str__

    # ---- catalogue ------------------------------------------------------------------------
    def search(self):
        """(ids, outputs-or-filenames, npackets, totalsource) of the runs made with these inputs
        (Input.py:121-172, without the database)."""
        runs = self._catalogue
        if not runs:
            return ([], [], 0, 0)
        return ([run.idnum for run in runs], [run.filename or run for run in runs],
                int(sum(run.npackets for run in runs)),
                float(sum(run.totalsource for run in runs)))

    def delete_files(self, filename=None):
        """Forget (and remove from disk) every catalogued run, or only the one saved as
        ``filename`` (Input.py:274-...)."""
        self.wait()
        doomed = [run for run in self._catalogue if filename is None or run.filename == filename]
        for run in doomed:
            if run.filename and os.path.exists(run.filename):
                os.remove(run.filename)
        self._catalogue = [run for run in self._catalogue if run not in doomed]
        self._fused = []

    def chunk_size(self, packs_per_it=None):
        """Packets per Output when the caller does not say (Input.py:216-227): a million for the
        adaptive driver; for the constant-step driver as many as keep the (N, 8, nsteps) history
        near 1024^3 doubles / 8."""
        if packs_per_it is not None:
            return int(packs_per_it)
        step = self.options.step_size
        if step == 0:
            return 1_000_000
        records = int(math.ceil(self.options.endtime.value/step) + 1)
        return int(math.ceil(1024**3/records/8))

    def run(self, npackets, packs_per_it=None, overwrite=False, compress=True,
            distribute=False, seed=None, *, device=0, keep_trajectory=True, context=None,
            sampler='numpy', batch=True, generator='philox', cp=None):
        """Integrate until the catalogue holds ``npackets`` packets (Input.py:175-268).

        Every pass plans ``ceil(todo / size)`` Outputs of ``size = min(todo, chunk_size)``
        packets -- the reference's arithmetic, so the last Output of a pass may overshoot
        (distributed.pass_plan).  With a ``seed`` the k-th Output of this call is drawn from
        ``seed + k``: Output 0 is the reference's stream; the reference itself passes the same
        seed to every Output (Input.py:246), which repeats identical packets.  ``sampler='device'``
        draws the initial states on the GPU instead, counter-based under the one ``seed`` or, with
        ``generator='pcg64'``, following the host's streams (the rule of each kind: draws.py).

        The Outputs of a pass are independent, so they are INTEGRATED TOGETHER (``batch``): one
        upload, one launch of each kernel over all their packets (Output.integrate_batch), each
        Output then owning its slice of the rows, which stay in HBM for produce_image /
        LOSResult.  With a ``savepath`` the files are written by a worker thread beside the next
        launch (``wait()`` joins it).

        ``cp`` (a distributed.ControlPlane of several ranks, one process per GPU): the run is
        SHARED.  The plan -- how many Outputs, of which size, from which seed or index range -- is
        the single-process plan; rank r makes the Outputs ``shard_range(passes, r, world)`` of
        every pass and catalogues only those, so Output k is the same Output whatever the number
        of ranks, and the union of the ranks' catalogues is the single-process catalogue.  The
        packet count that ends the run is summed over the ranks.  ``produce_image(..., cp=cp)`` and
        ``LOSResult.simulate_data_from_inputs(..., cp=cp)`` then sum over the ranks what the
        reference sums over the files (ModelImage.py:96-98, LOSResult.py:264-266)."""
        started = time.time()
        rank, world = (cp.rank, cp.world) if cp is not None else (0, 1)
        rule = Draws(sampler, generator, seed, cp)   # (an unseeded shared run agrees on a seed)

        def report():
            local = self._report()
            return local if world == 1 else int(round(cp.reduce(float(local), 'SUM')))
        if distribute in (True, 'delay', 'delayed'):
            assert False, 'Dont do this'         # the reference's dask path is disabled too
        if overwrite:
            self.delete_files()
        have = report()
        want = int(npackets)
        # re-emission draws are keyed by (the Output's seed, the packet's number): Outputs that
        # each have their own seed (host-sampled, or following the host streams with 'pcg64')
        # cannot share a launch when packets are re-emitted
        spec = self.surfaceinteraction
        sticks = spec.sticktype == 'constant' and spec.stickcoef == 1.
        together = bool(batch) and keep_trajectory and (compress or self.options.step_size == 0) \
            and (sticks or rule.one_key)
        if together and context is None:
            from . import hip_api
            context = hip_api.Context(device)

        def make(entry):
            # a planned Output: it draws for itself or, together, the device's launch group does
            return Output(self, entry.size, compress=compress, device=device, context=context,
                          keep_trajectory=keep_trajectory, integrate=not together,
                          save=not together, **rule.output_keywords(entry, presampled=together))

        made, drawn = 0, have                    # Outputs of this call; next free packet index
        while have < want:
            todo, passes, size, made, drawn = pass_plan(
                have, want, self.chunk_size(packs_per_it), made, drawn, rank, world)
            print('Running Model')
            print(f'Will complete {passes} iterations of {size} packets.')
            if world > 1:
                lo, hi = shard_range(passes, rank, world)
                print(f'Rank {rank} of {world}: iterations {lo + 1} to {hi}.')
            ahead, at = None, 0     # host-drawn Outputs on their way; next of ``todo`` to launch
            try:
                while at < len(todo):
                    tick = time.time()
                    # as many Outputs per launch as HBM takes (rows: nsteps records per packet at
                    # most, far fewer in practice; the row store spills its oldest runs to the host)
                    limit = self._group_limit(size, context) if together else 1
                    outs = []
                    if together and rule.on_host and (min(len(todo) - at, limit) > 1 or ahead):
                        # The Outputs are drawn on a few threads (NumPy releases the GIL in its
                        # loops) a window ahead of the device, and a launch takes what is drawn by
                        # the time the device is free: the first launch starts after the first
                        # draws instead of after a whole group's, later ones find Outputs waiting.
                        # A launch has a fixed cost of several milliseconds (two passes, row
                        # offsets, a store): the first takes a handful of Outputs so that the
                        # device starts early, the later ones wait for a third of what HBM takes
                        # (or the rest of the pass) and then add whatever else is drawn by then.
                        floor = max(1, min(limit, HOST_SAMPLER_THREADS)) if ahead is None else \
                            max(1, min(limit//3, HOST_SAMPLER_THREADS*2))
                        if ahead is None:
                            ahead = DrawAhead(lambda entry: make(entry).prepare_for_launch(),
                                              todo[at:], HOST_SAMPLER_THREADS)
                        window = max(2*HOST_SAMPLER_THREADS, 2*limit)
                        ahead.fill(window)
                        while ahead and len(outs) < floor:
                            outs.append(ahead.popleft().result())
                            ahead.fill(window)
                        while ahead and ahead[0].done() and len(outs) < limit:
                            outs.append(ahead.popleft().result())
                    else:
                        for entry in todo[at:at + limit]:
                            print(f'Starting iteration #{entry.number + 1} of {passes}')
                            outs.append(make(entry))
                            context = outs[-1].context()     # every Output shares one device
                    at += len(outs)
                    if together:
                        self._launch_group(outs, context, rule)
                    print(f'Completed iteration #{todo[at - 1].number + 1} in '
                          f'{time.time() - tick} seconds.')
            finally:
                if ahead is not None:
                    ahead.pool.shutdown(cancel_futures=True)
            have = report()
        self.wait()                              # files of this run are on disk when it returns
        print(f'Model run completed in {time.time() - started:.2f} sec.')

    def _launch_group(self, outs, context, rule):
        """Draw (device samplers) and integrate the Outputs ``outs`` in one launch.  If their rows
        turn out not to fit in HBM beside what is resident -- the estimate of _group_limit assumes
        typical lifetimes -- the group is split in halves and tried again."""
        from . import hip_api
        try:
            rule.fill_group(context, outs)
            Output.integrate_batch(outs, context)
        except hip_api.HipError as exc:
            if exc.code != hip_api.NXC_ERR_NOMEM or len(outs) < 2:
                raise
            half = len(outs)//2
            print(f'{len(outs)} Outputs in one launch need more HBM than is free: two launches')
            self._launch_group(outs[:half], context, rule)
            self._launch_group(outs[half:], context, rule)

    def _group_limit(self, size, context):
        """How many Outputs of ``size`` packets one launch may take: the packets' states and a
        generous estimate of their rows (a quarter of the dense history) within a third of the
        device's free memory; at least one."""
        step = self.options.step_size
        per_packet = 8*8*3
        if step != 0:
            records = int(math.ceil(self.options.endtime.value/step) + 1)
            per_packet += records*80//4
        free, _ = context.mem_info()
        return max(1, int(free//3//(per_packet*size)))

    # ---- files in the background ------------------------------------------------------------
    def _write_later(self, job, *args):
        """Run ``job(*args)`` on the writer thread (one at a time, in order)."""
        if getattr(self, '_writer', None) is None:
            from concurrent.futures import ThreadPoolExecutor
            self._writer, self._pending = ThreadPoolExecutor(max_workers=1), []
        self._pending.append(self._writer.submit(job, *args))

    def wait(self):
        """Block until every file of the catalogue is on disk; re-raises a writer's error."""
        pending, self._pending = getattr(self, '_pending', []), []
        for job in pending:
            job.result()

    def _report(self):
        _, files, packets, _ = self.search()
        print(f'Found {len(files)} files with {packets} packets.')
        return packets

    def produce_image(self, format_, overwrite=False, distribute=None, *, cp=None, reduce='rccl',
                      **kwargs):
        """Input.py:270-272.  ``cp``: the control plane of a shared run (``run(..., cp=cp)``):
        every rank bins the Outputs of its own catalogue and the image pairs and source totals
        are summed over the ranks (reduce='rccl': one ncclAllReduce; 'host': over the control
        plane, for tests) -- every rank gets the image of the whole run."""
        from .ModelImage import ModelImage, read_params, refuse_cube_with, refuse_moments_with
        if cp is not None:
            from .frames import is_planet_origin, refuse_with_moon_origin
            if not is_planet_origin(self, read_params(format_).get('origin')):
                refuse_with_moon_origin(cp=cp)
        if kwargs.get('ages') is not None:
            from .transient import refuse_ages_with
            refuse_ages_with(cp=cp, moments=kwargs.get('moments'), cube=kwargs.get('cube'))
        if kwargs.get('cube') is not None:
            refuse_cube_with(cp=cp, moments=kwargs.get('moments'))
        if kwargs.get('moments'):
            refuse_moments_with(cp=cp)
        if cp is None or cp.world == 1:
            return ModelImage(self, format_, overwrite=overwrite, distribute=distribute, **kwargs)
        from .distributed import guarded, merge_catalogue
        image = ModelImage(self, format_, overwrite=overwrite, distribute=distribute,
                           finalize=False, **kwargs)
        with guarded(cp, image.context()):
            merge_catalogue(image, cp, image.context(), reduce)
        image.finalize()
        return image
