"""A job's engine options in one place: which there are, which go together, what identifies an engine, and which engine keywords
a parsed job description means ("Where a job option lives")."""
from dataclasses import dataclass
from typing import FrozenSet, Optional, Tuple

from . import control as control_mod, hypertile as hypertile_mod, ipadapter as ipadapter_mod, reference as reference_mod, regions as regions_mod, samplers as smp
from . import t2iadapter as t2i_mod
from .engine import PAG_LAYERS

# job kind -> (what it is, the arguments and then the states it cannot be combined with, in the order the error names them)
REFUSED = {
    "regions": ("text-to-image on one stream only", ("tiled", "hires", "control_net_image", "reference_image", "inpaint_mask"),
                ("a TCD pipeline (active_tcd=True)", "denoise_streams = 2")),
    "tiled": ("text-to-image on the device loop only", ("reference_image", "inpaint_mask", "control_net_image", "hires"),
              ("host_loop=True", "a TCD pipeline (active_tcd=True)")),
    "hires": ("text-to-image on the device loop only", ("reference_image", "inpaint_mask", "control_net_image"),
              ("host_loop=True", "a TCD pipeline (active_tcd=True)")),
    "pag": ("text-to-image on one stream only", ("regions", "tiled", "hires", "control_net_image", "reference_image", "inpaint_mask"),
            ("denoise_streams = 2",)),
    "hypertile": ("text-to-image on one stream only", ("tiled", "regions", "pag", "reference_only", "control_net_image", "inpaint_mask",
                                                       "reference_image"), ("denoise_streams = 2",)),
    "reference_only": ("text-to-image on one stream only", ("regions", "pag", "tiled", "hires", "control_net_image", "reference_image",
                                                            "inpaint_mask"), ("a TCD pipeline (active_tcd=True)", "denoise_streams = 2")),
    "sag": ("text-to-image on one stream only",
            ("regions", "tiled", "hires", "pag", "reference_only", "hypertile", "control_net_image", "reference_image", "inpaint_mask"),
            ("denoise_streams = 2",)),
    "dynamic_threshold": ("guided text-to-image on one stream only", ("tiled", "control_net_image", "reference_image", "inpaint_mask"),
                          ("a TCD pipeline (active_tcd=True)", "denoise_streams = 2")),
}

# An engine's own refusal of a kind reads "<kind>: <what it is> (no <the excluded things an engine can see, in its words>)"; these two
# read otherwise and are kept whole
_ENGINE_SENTENCE = {
    "tiled": "tiled: text-to-image only (no ControlNet, inpainting or TCD)",
    "dynamic_threshold": "dynamic_threshold: guided text-to-image on one stream only (guidance > 0, no ControlNet, inpainting, TCD, tiled, denoise_streams = 2)",
}


def job_options(sampler=None, regions=None, pag=None, reference=None, hypertile=None, sag=None, dynthresh=None, control=None,
                ip_tokens=None, t2i_units=None) -> dict:
    """_engine's option keywords of a job from its parsed descriptions (None: the job has none): only what the job asks for.
    `control`: the parsed units of control.parse - the engine is built for their number only.  `ip_tokens`: the number of image
    tokens of a job with an IP-Adapter image prompt - the engine is built for that number only.  `t2i_units`: the number of
    T2I-Adapters of a job with t2i_adapter= - the engine is built for that number only."""
    out = dict(sampler=sampler and sampler.name, pag=pag and pag.key, hypertile=hypertile, sag=sag and True, dynthresh=dynthresh and True,
               control_units=control and len(control), ip_tokens=ip_tokens or None, t2i_units=t2i_units or None)
    if regions is not None:   # (the base prompt counts when it is evaluated)
        out.update(regions=regions.count, region_mode=regions.mode)
    if reference is not None:
        out.update(reference=tuple(sorted(reference.layers)), adain=reference.adain_key)
    return {k: v for k, v in out.items() if v is not None}


@dataclass(frozen=True)
class EngineOptions:
    """What a DenoiseEngine takes beyond shape and guidance, in the form its attributes of the same names have."""
    sampler: Optional[smp.SamplerSpec] = None        # a multistep / ancestral sampler of minsdtf_amd/samplers.py
    tiled: Optional[object] = None                   # the tiled.Geometry of a tiled job: the batch rows are its views
    regions: int = 0                                 # the number of evaluated region prompts
    region_mode: str = "latent"                      # "attention": the masks act inside every attn2; "latent" without regions
    pag: Optional[FrozenSet[str]] = None             # the attention blocks of a perturbed-attention-guidance job
    reference: Optional[FrozenSet[str]] = None       # the attention blocks of a reference-only job; empty beside AdaIN sites
    adain: Optional[FrozenSet[str]] = None           # the reference AdaIN sites of such a job
    hypertile: Optional[Tuple[int, ...]] = None      # (nh, nw, depth) of a HyperTile job
    sag: bool = False                                # self-attention guidance
    dynthresh: bool = False                          # dynamic thresholding
    control_units: int = 0                           # the number of ControlNet units of a job with control= (minsdtf_amd/control.py)
    ip_tokens: int = 0                               # the number of image tokens of a job with ip_adapter= (minsdtf_amd/ipadapter.py)
    t2i_units: int = 0                               # the number of adapters of a job with t2i_adapter= (minsdtf_amd/t2iadapter.py)

    @classmethod
    def of(cls, **opts) -> "EngineOptions":
        """From the keywords as a caller gives them; None and absent both mean the default.  TypeError for a name that is no option."""
        o = cls(**{k: v for k, v in opts.items() if v is not None})   # (the constructor's TypeError for an unknown name)
        regions, adain, ht = int(o.regions), frozenset(o.adain) if o.adain else None, o.hypertile
        return cls(sampler=smp.parse(o.sampler), tiled=o.tiled, regions=regions,
                   region_mode=o.region_mode if regions or o.region_mode not in regions_mod.MODES else "latent",   # (an unknown mode stays, for check() to name)
                   pag=frozenset(o.pag) if o.pag else None, reference=frozenset(o.reference or ()) if (o.reference or adain) else None,
                   adain=adain, hypertile=tuple(int(v) for v in ht) if ht is not None and len(ht) == 3 else ht,   # (else as given, for check())
                   sag=bool(o.sag), dynthresh=bool(o.dynthresh), control_units=int(o.control_units), ip_tokens=int(o.ip_tokens),
                   t2i_units=int(o.t2i_units))

    def key(self) -> tuple:
        """What the options add to an engine's key behind the UNet-size part: what the plans depend on, nothing a call uploads."""
        key = () if self.tiled is None else (self.tiled.key,)   # (a tiled job: B counts views)
        if self.regions:
            key += (("regions", self.regions) + (("attention",) if self.region_mode == "attention" else ()),)
        if self.pag:
            key += (("pag", tuple(sorted(self.pag))),)
        if self.reference is not None:   # (with reference AdaIN the site set too, behind the blocks - which may then be none)
            key += (("reference", tuple(sorted(self.reference))) + ((("adain",) + tuple(sorted(self.adain)),) if self.adain else ()),)
        key += ((("hypertile",) + self.hypertile,) if self.hypertile else ()) + ((("sag",),) if self.sag else ())
        key += (("dynthresh",),) if self.dynthresh else ()
        key += (("control", self.control_units),) if self.control_units else ()
        key += (("ip", self.ip_tokens),) if self.ip_tokens else ()
        return key + ((("t2i", self.t2i_units),) if self.t2i_units else ())

    def check(self, h: int, w: int, B: int, guidance: float, control: bool, inpaint: bool, tcd: bool, streams) -> None:
        """ValueError for what an engine of batch B at h x w refuses: each kind's own checks, then its exclusions, read from REFUSED."""
        # (argument or state of REFUSED, the word an engine's refusal has for it, whether this engine sees it), in the order a
        # refusal names them; `hires`, `reference_image` and `host_loop=True` have no engine form: an engine never meets them
        seen = (("control_net_image", "ControlNet", control), ("inpaint_mask", "inpainting", inpaint), ("a TCD pipeline (active_tcd=True)", "TCD", tcd),
                ("tiled", "tiled", self.tiled is not None), ("regions", "regions", self.regions), ("pag", "pag", self.pag),
                ("reference_only", "reference_only", self.reference is not None), ("hypertile", "hypertile", self.hypertile is not None),
                ("sag", "sag", self.sag), ("denoise_streams = 2", "denoise_streams = 2", streams == 2))

        def exclusive(kind, asked=True, also=False):
            what, arguments, states = REFUSED[kind]
            named = [(word, holds) for name, word, holds in seen if name in arguments + states]
            if asked and (also or any(holds for _word, holds in named)):
                raise ValueError(_ENGINE_SENTENCE.get(kind) or f"{kind}: {what} (no {', '.join(word for word, _holds in named)})")

        def known(kind, what, names, allowed):
            if set(names or ()) - set(allowed):
                raise ValueError(f"{kind}: unknown {what} {sorted(set(names) - set(allowed))}")

        if self.sampler is not None and tcd:
            raise ValueError("a sampler cannot be combined with the TCD sampler")
        if self.tiled is not None:
            if (self.tiled.th, self.tiled.tw) != (h, w) or B % self.tiled.views:
                raise ValueError(f"tiled: {self.tiled.views} views of {self.tiled.th} x {self.tiled.tw} on an engine of batch {B} at {h} x {w}")
            exclusive("tiled")
        if self.region_mode not in regions_mod.MODES:
            raise ValueError(f"regions: mode = {self.region_mode!r}: one of {regions_mod.MODES}")
        if self.regions:
            if not 1 <= self.regions <= regions_mod.MAX_REGIONS:
                raise ValueError(f"regions: {self.regions} region prompts (1 .. {regions_mod.MAX_REGIONS})")
            exclusive("regions")
        known("pag", "layer(s)", self.pag, PAG_LAYERS)
        exclusive("pag", self.pag)
        if self.reference is not None:
            known("reference_only", "layer(s)", self.reference, PAG_LAYERS)
            known("reference_only", "adain site(s)", self.adain, [n for n, _gw in reference_mod.ADAIN_SITES])
            exclusive("reference_only")
        if self.hypertile is not None:
            if len(self.hypertile) != 3:
                raise ValueError(f"hypertile: {self.hypertile!r} is not (nh, nw, depth)")
            hypertile_mod.level_geometry(h, w, *self.hypertile)   # (ValueError for windows the levels cannot take)
            exclusive("hypertile")
        exclusive("sag", self.sag)
        exclusive("dynamic_threshold", self.dynthresh, also=not guidance > 0.0)
        # control units exclude nothing a ControlNet job is not already excluded from (the rows above name it): no REFUSED row
        if self.control_units and not (1 <= self.control_units <= control_mod.MAX_UNITS and control):
            raise ValueError(f"control: {self.control_units} unit(s) (1 .. {control_mod.MAX_UNITS}, on an engine with a ControlNet)")
        # an image prompt's exclusions live in ipadapter.py (REFUSED above is counted by its tests): no REFUSED row either
        if self.ip_tokens:
            if not 1 <= self.ip_tokens <= ipadapter_mod.MAX_TOKENS:
                raise ValueError(f"ip_adapter: {self.ip_tokens} image tokens (1 .. {ipadapter_mod.MAX_TOKENS})")
            ipadapter_mod.refuse(dict(regions=self.regions or None, pag=self.pag, sag=self.sag or None, reference_only=self.reference,
                                      hypertile=self.hypertile, tiled=self.tiled), streams)
        # a T2I-Adapter's exclusions live in t2iadapter.py, like the image prompt's: no REFUSED row
        if self.t2i_units:
            if not 1 <= self.t2i_units <= t2i_mod.MAX_UNITS:
                raise ValueError(f"t2i_adapter: {self.t2i_units} units (1 .. {t2i_mod.MAX_UNITS})")
            t2i_mod.check_size(8 * h, 8 * w)
            t2i_mod.refuse(dict(control_net_image=control or None, regions=self.regions or None, pag=self.pag, sag=self.sag or None,
                                reference_only=self.reference, hypertile=self.hypertile, tiled=self.tiled), streams)
