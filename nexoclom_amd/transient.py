"""Images for a source whose rate changes with time: the host side of ``ages=``.

Every product reads the stored rows as a steady state: a row at t_remaining = t is a packet of age
t0 - t (t0 = options.endtime), and the image sums over all ages.  A row of age a stands for atoms
launched a seconds before the epoch, so the image is linear in the source's history.  An object
built with ``ages=(a_lo_s, a_hi_s, nbins)`` files every sample's weight under its age as well as its
pixel (k_image_ages / k_camera_ages; include/nexoclom_hip.h, "Age cube"): the planes of that cube
are the image's response to a pulse of the source rate, and the image at an epoch t_e for a source
whose rate was ``rate(t)`` times the nominal one is

    image(t_e)[pix] = sum_k  cube[pix][k] * mean of rate over the launch times of age bin k

-- one contraction of the cube with a small matrix (``response_matrix``; k_ages_apply on the
device).  Only the rate changes: where and how fast the source launches stays as the run had it.
LOSResult files the pairs of its lines of sight and ModelDensity the members of its points' balls
the same way; their ``transient`` reads each spectrum or point at an epoch of its own.  ShellMap
files both records of a sample (k_shell_ages); its ``transient`` gives the shells per epoch.
Host only, NumPy only."""
import operator

import numpy as np


def parse_ages(ages):
    """``(a_lo_s, a_hi_s, nbins)`` of an ``ages=`` argument as (float, float, int); ValueError
    for anything but three numbers, a bin count that is no positive integer, or a range that is
    empty or not finite."""
    try:
        a_lo, a_hi, nbins = ages
        a_lo, a_hi = float(a_lo), float(a_hi)
    except (TypeError, ValueError):
        raise ValueError('ages= takes three numbers (a_lo_s, a_hi_s, nbins)') from None
    try:
        nbins = operator.index(nbins)
    except TypeError:
        raise ValueError('ages=: the number of bins must be an integer') from None
    if nbins < 1:
        raise ValueError('ages=: the number of bins must be at least 1')
    if not (np.isfinite(a_lo) and np.isfinite(a_hi) and np.isfinite(a_hi - a_lo)):
        raise ValueError('ages=: the age range must be finite')
    if not a_lo < a_hi:
        raise ValueError('ages=: the age range is empty (a_lo_s must be below a_hi_s)')
    return a_lo, a_hi, nbins


def refuse_ages_with(**given):
    """NotImplementedError for what an ages pass cannot be combined with."""
    why = {'npackets': 'ages= reads catalogued Outputs only: streaming (npackets=) bins inside the '
                       'fused integrate kernel, which carries no age block',
           'shard': 'ages= does not support shard=: the age sums are not reduced over shards',
           'cp': 'ages= does not support cp=: there is no all-reduce of the age sums yet',
           'moments': 'ages= does not support moments=True: each is a pass of its own that adds to '
                      'the same sums, so two passes would add them twice; make two objects',
           'cube': 'ages= does not support cube=: each is a pass of its own that adds to the '
                   'image, so two passes would add it twice; make two objects',
           'profile': 'ages= does not support profile=: a line-of-sight pass files its pairs by '
                      'age or by velocity, not both; make two objects',
           'spectrum': 'ages= does not support spectrum=: each is a pass of its own that adds to '
                       'the density, so two passes would add it twice; make two objects'}
    for key, value in given.items():
        if value is not None and value is not False:
            raise NotImplementedError(why[key])


def refuse_ages_of(inputs):
    """NotImplementedError for inputs whose row stores do not carry the age."""
    if inputs.options.step_size == 0:
        raise NotImplementedError(
            'ages= needs a constant-step run: with step_size = 0 the row store holds only each '
            'packet\'s final row at t_remaining ~ 0, so it does not carry the age')


def new_age_sums(dims, ages):
    """Zeroed ``age_sums`` for an image of ``dims`` pixels; ValueError when the block has more
    records than the device addresses (nx nz (nbins + 2) < 2^31)."""
    if dims[0]*dims[1]*(ages[2] + 2) >= 2**31:
        raise ValueError('ages=: dims[0]*dims[1]*(nbins + 2) must stay below 2^31')
    return np.zeros(tuple(dims) + (ages[2] + 2, 2))


def ages_from_sums(age_sums, atoms_per_packet, a_lo, a_hi):
    """What an ages pass publishes, from ``age_sums`` (nx, nz, nbins + 2, 2) = {sum w, sum w w} per
    pixel and plane (plane 0 younger than the range, 1..nbins the bins, nbins + 1 at or above it):
      age_cube, age_below, age_above  sum w times ``atoms_per_packet``, the image's scaling
      age_edges, age_axis             a_lo + k (a_hi - a_lo)/nbins and the bins' centres [s]
      age_effective_packets           (sum w)^2 / sum w w per bin, 0 where a bin is empty"""
    age_sums = np.asarray(age_sums, dtype=float)
    nbins = age_sums.shape[-2] - 2
    S, ww = age_sums[..., 1:-1, 0], age_sums[..., 1:-1, 1]
    filled = ww != 0
    edges = a_lo + np.arange(nbins + 1)*(a_hi - a_lo)/nbins
    return {'age_cube': S*atoms_per_packet,
            'age_below': age_sums[..., 0, 0]*atoms_per_packet,
            'age_above': age_sums[..., -1, 0]*atoms_per_packet,
            'age_edges': edges,
            'age_axis': (edges[:-1] + edges[1:])/2,
            'age_effective_packets': np.where(filled, S*S/np.where(filled, ww, 1.0), 0.0)}


def _history(history):
    try:
        nodes, rates = history
        nodes = np.atleast_1d(np.asarray(nodes, dtype=float))
        rates = np.atleast_1d(np.asarray(rates, dtype=float))
    except (TypeError, ValueError):
        raise ValueError('history is (t_nodes_s, rate_nodes): two sequences of numbers') from None
    if nodes.ndim != 1 or rates.shape != nodes.shape or nodes.size < 1:
        raise ValueError('history: t_nodes_s and rate_nodes are two 1-d sequences of one length')
    if not np.all(np.isfinite(nodes)) or not np.all(np.diff(nodes) > 0):
        raise ValueError('history: the nodes must be finite and strictly increasing')
    if not np.all(np.isfinite(rates)) or np.any(rates < 0):
        raise ValueError('history: the rates must be finite and >= 0')
    return nodes, rates


def _mean_rate(p, q, nodes, rates):
    """The exact mean over [p, q] (arrays; either order) of the function that is piecewise linear
    through (nodes, rates) and held at its end values outside them; its value at p where p == q.
    The interval is cut at the nodes and every piece, on which the function is linear, integrated
    in closed form: length times the mean of its two end values.  The pieces are summed as
    deviations from the value at p, so a constant history gives that constant exactly."""
    p, q = np.minimum(p, q), np.maximum(p, q)
    rate = lambda t: np.interp(t, nodes, rates)                         # noqa: E731
    ref = rate(p)
    total = np.zeros(p.shape)
    cuts = np.concatenate([[-np.inf], nodes, [np.inf]])
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        a, b = np.clip(p, lo, hi), np.clip(q, lo, hi)
        total += (b - a)*((rate(a) + rate(b))/2 - ref)
    width = q - p
    some = width > 0
    return np.where(some, ref + total/np.where(some, width, 1.0), ref)


def response_matrix(age_edges, epochs, history):
    """K (nbins + 2, E): what every plane of an age cube is multiplied with to give the image at
    each of the ``epochs`` [s] for the source ``history = (t_nodes_s, rate_nodes)``, the source
    rate relative to the nominal one (1 = the steady state the plain image assumes) -- piecewise
    linear in its nodes, held at its end values outside them, on the epochs' clock.

      row 1 + k   the mean of the rate over the launch interval of age bin k,
                  [t_e - age_edges[k + 1], t_e - age_edges[k]]
      row 0       (ages below age_edges[0]) the mean over [t_e - age_edges[0], t_e]; with
                  age_edges[0] == 0 the rate at t_e
      last row    (ages at or above age_edges[-1]) the first node's rate: the rate long ago

    The means are exact (closed form per linear piece, no sampling).  ValueError: age_edges that
    are not at least two finite, strictly increasing numbers; epochs that are not finite; nodes
    that are not finite and strictly increasing; rates that are not finite and >= 0."""
    try:
        edges = np.asarray(age_edges, dtype=float)
        epochs = np.atleast_1d(np.asarray(epochs, dtype=float))
    except (TypeError, ValueError):
        raise ValueError('age_edges and epochs are sequences of numbers') from None
    if edges.ndim != 1 or edges.size < 2 or not np.all(np.isfinite(edges)) or \
            not np.all(np.diff(edges) > 0):
        raise ValueError('age_edges: at least two finite, strictly increasing numbers')
    if epochs.ndim != 1 or epochs.size < 1 or not np.all(np.isfinite(epochs)):
        raise ValueError('epochs: one or more finite numbers')
    nodes, rates = _history(history)
    K = np.empty((edges.size + 1, epochs.size))
    K[0] = _mean_rate(epochs - edges[0], epochs, nodes, rates)
    K[1:-1] = _mean_rate(epochs[None, :] - edges[1:, None], epochs[None, :] - edges[:-1, None],
                         nodes, rates)
    K[-1] = rates[0]
    return K


class TransientImages:
    """What ``image.transient(epochs, history)`` returns:

      epochs             (E,) [s]
      kernel             (nbins + 2, E): the response matrix used
      images             (E, nx, nz), scaled as ``image`` is
      effective_packets  (E, nx, nz): (sum)^2 / (ww sum), 0 where a pixel is empty -- the error
                         bars are images / sqrt(effective_packets)
      light_curve        (E,): the sum over the pixels"""

    def __init__(self, epochs, kernel, sums, atoms_per_packet):
        self.epochs = np.atleast_1d(np.asarray(epochs, dtype=float))
        self.kernel = kernel
        S, ww = sums[..., 0], sums[..., 1]
        filled = ww != 0
        self.images = S*atoms_per_packet
        self.effective_packets = np.where(filled, S*S/np.where(filled, ww, 1.0), 0.0)
        self.light_curve = self.images.sum(axis=(1, 2))


def spectrum_times(times, default, n_spectra):
    """(S,) epochs of ``n_spectra`` spectra from ``times``: one per spectrum, one number for all of
    them, or -- None -- ``default`` (the spacecraft data's ``time`` column).  ValueError when there
    is neither, for another length and for a time that is not finite."""
    if times is None:
        if default is None:
            raise ValueError('transient: times is missing and the spacecraft data had no time '
                             'column')
        times = default
    try:
        times = np.asarray(times, dtype=float)
    except (TypeError, ValueError):
        raise ValueError('transient: times are numbers') from None
    if times.ndim == 0:
        times = np.full(n_spectra, float(times))
    if times.shape != (n_spectra,):
        raise ValueError(f'transient: times of shape {times.shape} for {n_spectra} spectra')
    if not np.all(np.isfinite(times)):
        raise ValueError('transient: all times must be finite')
    return times


class TransientRadiance:
    """What ``los.transient(history, times)`` returns:

      times              (S,) [s]: the epoch of every spectrum
      kernel             (nbins + 2, S): column s is the response at the epoch of spectrum s
      radiance           (S,) Series [kR], indexed like the result's ``radiance``:
                         sum_k S[s][k] K[k][s]
      effective_packets  (S,) Series: (sum)^2 / sum_k WW[s][k] K[k][s]^2, 0 where a spectrum is
                         empty -- the error bars are radiance / sqrt(effective_packets)

    Both sums run over k = 0 .. nbins + 1 in that order from 0.0, one rounding per operation: a
    pure function of ``age_sums`` and the kernel."""

    def __init__(self, times, age_edges, history, age_sums, scale, rows):
        import pandas as pd
        self.times = times
        self.kernel = K = response_matrix(age_edges, times, history)
        total, effective = track_sums(age_sums, K)
        self.radiance = pd.Series(total*scale, index=rows)
        self.effective_packets = pd.Series(effective, index=rows)


def track_sums(age_sums, K):
    """(sum_k S[n][k] K[k][n], its effective packets) per record n of ``age_sums`` (N, nbins + 2,
    2) read with its own column of ``K`` (nbins + 2, N): both sums over k = 0 .. nbins + 1 in that
    order from 0.0, one rounding per operation; the effective packets are (sum)^2 /
    sum_k WW[n][k] K[k][n]^2, 0 where a record is empty."""
    total, ww = np.zeros(K.shape[1]), np.zeros(K.shape[1])
    for k in range(K.shape[0]):
        total = total + age_sums[:, k, 0]*K[k]
        ww = ww + age_sums[:, k, 1]*(K[k]*K[k])
    filled = ww != 0
    return total, np.where(filled, total*total/np.where(filled, ww, 1.0), 0.0)


class TransientDensity:
    """What ``dens.transient(epochs, history)`` returns:

      epochs             (E,) [s]
      kernel             (nbins + 2, E): the response matrix used
      density            (E, Q), scaled as ``density`` is
      effective_packets  (E, Q): (sum)^2 / (ww sum), 0 where a point is empty -- the error bars
                         are density / sqrt(effective_packets)"""

    def __init__(self, epochs, kernel, sums, scale):
        self.epochs = np.atleast_1d(np.asarray(epochs, dtype=float))
        self.kernel = kernel
        S, ww = sums[..., 0], sums[..., 1]
        filled = ww != 0
        self.density = S*scale
        self.effective_packets = np.where(filled, S*S/np.where(filled, ww, 1.0), 0.0)


class TransientTrack:
    """What ``dens.transient_track(history, times)`` returns:

      times              (Q,) [s]: the epoch of every point
      kernel             (nbins + 2, Q): column q is the response at the epoch of point q
      density            (Q,), scaled as ``density`` is: scale * sum_k S[q][k] K[k][q]
      effective_packets  (Q,): ``track_sums``' -- the error bars are density /
                         sqrt(effective_packets)"""

    def __init__(self, times, age_edges, history, age_sums, scale):
        self.times = times
        self.kernel = response_matrix(age_edges, times, history)
        total, self.effective_packets = track_sums(age_sums, self.kernel)
        self.density = total*scale


class TransientShells:
    """What ``shell.transient(epochs, history)`` returns, from ``sums`` (2, E, nlon, nlat, nalt + 2,
    2), both planes of the shell map's age block contracted with the kernel ({sum_k S K,
    sum_k WW K K} per epoch, cell and altitude record):

      epochs                     (E,) [s]
      kernel                     (nbins + 2, E): the response matrix used
      density                    (E, nlon, nlat, nalt), scaled as the map's ``density`` is
      column_profile             (E, nlon, nlat, nalt), scaled as ``column`` is
      column                     (E, nlon, nlat): plane B summed over all nalt + 2 records of a
                                 cell from record 0 upwards, scaled as ``column`` is
      density_effective_packets  (E, nlon, nlat, nalt): (sum)^2 / (ww sum), 0 where empty
      column_effective_packets   (E, nlon, nlat): the same of the cell's sums
      content                    (E,): for 'column' the atoms inside the altitude range,
                                 atoms_per_packet times plane A's sums over the bins 1..nalt of all
                                 cells; None for 'radiance'"""

    def __init__(self, epochs, kernel, sums, atoms_per_packet, solid_angle, volume, R_cm,
                 quantity='column'):
        self.epochs = np.atleast_1d(np.asarray(epochs, dtype=float))
        self.kernel = kernel
        sums = np.asarray(sums, dtype=float)
        A, B = sums[0][..., 1:-1, :], sums[1]
        per_area = atoms_per_packet/(solid_angle*R_cm**2)
        cell = np.zeros(B.shape[:3] + (2,))
        for k in range(B.shape[3]):
            cell = cell + B[:, :, :, k]

        def effective(S, ww):
            filled = ww != 0
            return np.where(filled, S*S/np.where(filled, ww, 1.0), 0.0)

        self.density = A[..., 0]*atoms_per_packet/(np.asarray(volume)*R_cm**3)
        self.column_profile = B[..., 1:-1, 0]*per_area
        self.column = cell[..., 0]*per_area
        self.density_effective_packets = effective(A[..., 0], A[..., 1])
        self.column_effective_packets = effective(cell[..., 0], cell[..., 1])
        self.content = atoms_per_packet*A[..., 0].sum(axis=(1, 2, 3)) if quantity == 'column' \
            else None
