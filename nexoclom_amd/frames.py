"""Moon-centred frames: the moons of a run, and the frame that co-rotates with one of them.

A constant-step run stores every step of every packet, and the stored-sample products read a row
at ``t_remaining = t`` as a packet of age ``t0 - t`` seen at the epoch ``t_remaining = 0``.  That
steady-state reading holds in a frame in which the source stands still; for a run launched from a
moon that is the frame which co-rotates with the moon.  ``MoonFrame`` holds what
include/nexoclom_hip.h ("Moon-centred frame") defines: the rotation rate, the moon's position and
velocity at the epoch and the scale to moon radii.  ``hip_api.Context.frame_rows`` /
``frame_columns`` move rows into it (k_frame_rows), and ``catalogue.sample_pass(..., frame=)``
hands the moved rows to a product's own kernel.
"""
import numpy as np


def moon_table(geometry, unit_km):
    """The included moons of ``geometry`` in the order of ``planet.moons`` (geometry.phi follows
    it), lengths in the planet's radius ``unit_km``: dicts of name, gm [R^3/s^2, negative],
    radius [R], a [R], omega [rad/s] and phi [rad at t_remaining = 0]."""
    planet = geometry.planet
    included = [m for m in (planet.moons or []) if m in (geometry.objects or ())]
    phis = [float(p) for p in (getattr(geometry, 'phi', None) or ())]
    assert len(phis) == len(included), 'The wrong number of orbital positions was given.'
    unit_m = unit_km*1e3
    return [dict(name=m.object, gm=m.GM.value/unit_m**3, radius=m.radius.value/unit_km,
                 a=m.a.value/unit_km, omega=2*np.pi/(m.orbperiod.value*86400.), phi=phi)
            for m, phi in zip(included, phis)]


class MoonFrame:
    """The frame that co-rotates with one moon of a run, centred on it, in moon radii.

    ``omega`` [rad/s], ``M`` = a (-sin phi, cos phi, 0) [R] and ``U`` = a omega (-cos phi,
    -sin phi, 0) [R/s], the moon's position and velocity at t_remaining = 0, ``scale`` = 1/rad
    (R per moon radius, inverted): the fields of nxc_frame_desc, formed here in fp64.
    ``origin`` is the moon's SSObject, ``unit`` / ``unit_km`` its radius as a length unit, and
    ``radvel_shift_kms`` is U_y in km/s: the Sun-relative radial velocity of a moved row is
    ``vy' + (vrplanet + U_y)``, so a consumer adds the shift to the vrplanet [km/s] it is set
    with."""

    def __init__(self, origin, moon, planet_km):
        self.origin = origin
        self.name = moon['name']
        self.omega = float(moon['omega'])
        a, phi = float(moon['a']), float(moon['phi'])
        self.M = np.array([-a*np.sin(phi), a*np.cos(phi), 0.0])
        self.U = np.array([-a*self.omega*np.cos(phi), -a*self.omega*np.sin(phi), 0.0])
        self.scale = 1.0/float(moon['radius'])
        self.unit = 'R_' + self.name
        self.unit_km = float(origin.radius.value)
        self.radvel_shift_kms = float(self.U[1])*float(planet_km)

    @classmethod
    def from_inputs(cls, inputs, origin):
        """The frame of ``origin`` -- a name ('Io') or an SSObject -- among the moons of
        ``inputs.geometry.objects``; ValueError when it is not one of them."""
        geometry = inputs.geometry
        name = getattr(origin, 'object', origin)
        name = name.strip().title() if isinstance(name, str) else name
        planet_km = float(geometry.planet.radius.value)
        moons = moon_table(geometry, planet_km) if getattr(geometry, 'phi', None) else []
        moon = next((m for m in moons if m['name'] == name), None)
        if moon is None:
            raise ValueError(f'origin {name!r} is not a moon among geometry.objects of these '
                             f'inputs (moons: {[m["name"] for m in moons] or "none"})')
        body = next(m for m in geometry.planet.moons if m.object == name)
        return cls(body, moon, planet_km)

    def __repr__(self):
        return f'MoonFrame({self.name})'


def is_planet_origin(inputs, origin):
    """Whether ``origin`` (None, a name or an SSObject) is the planet of ``inputs``."""
    if origin is None:
        return True
    name = getattr(origin, 'object', origin)
    if isinstance(name, str):
        name = name.strip().title()
    return name == inputs.geometry.planet.object


def refuse_with_moon_origin(**given):
    """NotImplementedError for what a moon-centred product cannot be combined with."""
    why = {'npackets': 'a moon origin reads catalogued Outputs only: streaming (npackets=) bins '
                       'inside the fused integrate kernel, which bins in the planet\'s frame',
           'shard': 'a moon origin does not support shard=: shards belong to the streaming pass, '
                    'which bins in the planet\'s frame',
           'cp': 'a moon origin does not support cp=: shared runs have not been tested in a '
                 'moon\'s frame'}
    for key, value in given.items():
        if value is not None:
            raise NotImplementedError(why[key])
