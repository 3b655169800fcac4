"""Python mirror of the reference's Renderer / Pass API over the C ABI.

Same names, argument meaning and state machine as src/renderer.ts and src/passes/*.ts
so that tests read like the reference's call sites (src/main.ts:374-400):

    renderer = Renderer.create()
    renderer.resize(1920, 1080); renderer.scalingFactor = 1
    renderer.setUniforms("raytrace", {"maxBounces": 8, "envMapIntensity": 1.0})
    scene.needsUpdate = True
    renderer.render(scene, camera)          # one frame: raytrace + accumulate + fullscreen

Everything that computes pixels happens in libmi3pt.so on the GPU; this file only
keeps the host-side state the reference keeps in TypeScript (frame counter, uniform
views, events).  The Node host in webgpu-pathtracer_amd/js mirrors the same API in
JavaScript for the N-API path.
"""
import math

import numpy as np

from . import capi, layout


class RollingAverage:
    """timing.ts:1-20"""

    def __init__(self, num_samples=30):
        self.num_samples = num_samples
        self.samples = []
        self.cursor = 0
        self.total = 0.0

    def addSample(self, v):
        old = self.samples[self.cursor] if self.cursor < len(self.samples) else 0.0
        self.total += v - old                      # one rounding, like `total += v - (samples[cursor] || 0)`
        if self.cursor < len(self.samples):
            self.samples[self.cursor] = v
        else:
            self.samples.append(v)
        self.cursor = (self.cursor + 1) % self.num_samples

    @property
    def value(self):
        return self.total / len(self.samples) if self.samples else float("nan")     # 0 / 0 before the first sample


class RaytracingScene:
    """scene.ts:3-5 plus what RaytracePass.updateScene needs: a flattened scene
    (mi3pt_host.scenes.Scene) and an optional 1024x512 float environment."""

    def __init__(self, content=None, environment=None):
        self.content = content
        self.environment = environment
        self.needsUpdate = False


class RaytracingCamera:
    """scene.ts:7-10 (PerspectiveCamera subset: fov in degrees, position, target)"""

    def __init__(self, fov=45.0, position=(0.0, 1.0, 4.0), target=(0.0, 0.0, 0.0)):
        self.fov = fov
        self.position = tuple(position)
        self.target = tuple(target)
        self.focalDistance = 1.0
        self.aperture = 0.0

    def getWorldPosition(self):
        return self.position

    def getWorldDirection(self):
        d = np.array(self.target, np.float64) - np.array(self.position, np.float64)
        return tuple(d / math.sqrt(float(d @ d)))


class Pass:
    """pass.ts:4-27"""

    def __init__(self, renderer):
        self.renderer = renderer
        self.timingAverage = RollingAverage()

    def updateTimings(self):
        if not self.renderer.options["enableTimestampQuery"]:
            return
        try:
            us = self.renderer.ctx.pass_time_us(self.PASS_ID)
        except capi.Mi3ptError as e:
            if e.code == 4:       # pass not timed in the last submit (fused into the raytrace kernel)
                return
            raise
        self.timingAverage.addSample(us)


class RaytracePass(Pass):
    PASS_ID = capi.PASS_RAYTRACE

    def __init__(self, renderer):
        super().__init__(renderer)
        self.uniforms = layout.UniformBlock(layout.RAYTRACE_UNIFORMS)
        self._nodesUploaded = 0                   # records of the tree the device holds
        self._builtNodes = self._builtCost = None     # the last FULL build's records, and their host_bvh_cost once it was needed

    def setUniforms(self, value):                 # raytrace.ts:359-369
        self.uniforms.set(value)
        self.renderer.ctx.set_uniforms(self.PASS_ID, self.uniforms.tobytes())

    def update(self):                             # raytrace.ts:371-378
        r = self.renderer
        # (_seedOffset: 0 unless reproject() was ever called -- a new view's samples must not replay the old view's random sequences)
        self.setUniforms({"resolution": [r.scaledWidth, r.scaledHeight], "aspect": r.aspect,
                          "frame": (r.frame + r._seedOffset) & 0xFFFFFFFF, "samplesPerFrame": r.samplesPerFrame})

    def updateScene(self, scene, camera):         # raytrace.ts:380-533
        self.setUniforms({"camera": {"position": camera.getWorldPosition(),
                                     "direction": camera.getWorldDirection(),
                                     "fov": camera.fov, "focalDistance": camera.focalDistance,
                                     "aperture": camera.aperture}})
        if not scene.needsUpdate:
            return
        if scene.environment is not None:
            self.renderer.updateEnvironmentTexture(scene.environment)
        content = scene.content
        if content is None or len(content.triangles) == 0:
            raise capi.Mi3ptError(1, "Input nodes array is empty")      # raytrace.ts:563-565
        ctx = self.renderer.ctx
        if not (self.renderer.refit and self._refitScene(content)):
            builder = self._deviceBuilder() if content.nodes is None else None
            if builder:
                # options["deviceBvh"]: the tree is built on the GPU from the uploaded triangles -- also the rebuild a refit above
                # refitCostLimit falls back to, which is what makes a finite limit affordable; lastRefitMs then reports that build
                ctx.upload_triangles(content.triangles)
                content.nodes, info = ctx.device_build_bvh(*builder)
                if self.renderer.lastRefitCostRatio is not None:
                    self.renderer.lastRefitMs = info.build_ms
                ctx.upload_bvh(content.nodes)
            else:
                if content.nodes is None:
                    content.build_bvh()
                ctx.upload_bvh(content.nodes)
                ctx.upload_triangles(content.triangles)
            self._builtNodes, self._builtCost = content.nodes, None
        self._nodesUploaded = len(content.nodes)
        ctx.upload_materials(content.material_bytes)
        scene.needsUpdate = False
        self.renderer._sceneVersion += 1
        self.renderer._trianglesUploaded = len(content.triangles)      # (reprojectScene: the count the next scene must have)

    def _deviceBuilder(self):
        """options["deviceBvh"]: False / absent (the default: the reference's SAH tree, built on the host), True or "lbvh" (the linear
        BVH, csrc/pt_lbvh.hip), "ploc" (the locally-ordered clustering of include/mi3pt.h, csrc/pt_ploc.hip, with
        options["deviceBvhRadius"], default 16) -> None, or the arguments of Context.device_build_bvh"""
        opt = self.renderer.options
        which = opt.get("deviceBvh", False)
        if which is None or which is False:
            return None
        method = "lbvh" if which is True else which
        if method not in capi.BVH_METHODS:
            raise ValueError(f"options['deviceBvh'] = {which!r}: expected True, 'lbvh' or 'ploc'")
        return (method, int(opt.get("deviceBvhRadius", 16)))

    def _refitScene(self, content):
        """renderer.refit (no counterpart in the reference, which rebuilds on every scene.needsUpdate, raytrace.ts:380-533): when only
        vertices moved -- the triangle count is the last upload's and a tree is uploaded -- the triangles go up first, the device re-fits
        the boxes of the uploaded tree to them (include/mi3pt.h: mi3pt_device_refit_bvh: the exact boxes of the old topology) and those
        records are uploaded and become content.nodes.  The price is tree quality: capi.host_bvh_cost of the result over that of the last
        full build is renderer.lastRefitCostRatio; above renderer.refitCostLimit (default inf: never) the caller rebuilds as it always
        did.  True when the tree and the triangles are uploaded.  Either way a tree the caller supplied in content.nodes is not used: it is
        replaced by the re-fitted records, or, above the limit, dropped (content.nodes = None) so that the caller builds the SAH tree of the new
        positions -- the only tree the cost recorded at "the last full build" can stand for."""
        r = self.renderer
        r.lastRefitCostRatio = r.lastRefitMs = None
        if not self._nodesUploaded or self._builtNodes is None or len(content.triangles) != r._trianglesUploaded:
            return False
        ctx = r.ctx
        ctx.upload_triangles(content.triangles)
        nodes, ms = ctx.device_refit_bvh()
        if self._builtCost is None:
            self._builtCost = capi.host_bvh_cost(self._builtNodes)
        cost = capi.host_bvh_cost(nodes)
        r.lastRefitMs = ms
        r.lastRefitCostRatio = cost / self._builtCost if self._builtCost > 0 else (math.inf if cost > 0 else 1.0)
        if r.lastRefitCostRatio > r.refitCostLimit:
            content.nodes = None                  # (whatever the content carried is not the tree of these positions: build)
            return False
        ctx.upload_bvh(nodes)
        content.nodes = nodes
        return True

    def render(self, encoder):                    # raytrace.ts:696-708
        encoder.append(capi.SUBMIT_RAYTRACE)


class AccumulatePass(Pass):
    PASS_ID = capi.PASS_ACCUMULATE

    def __init__(self, renderer):
        super().__init__(renderer)
        self.uniforms = layout.UniformBlock(layout.ACCUMULATE_UNIFORMS)

    def setUniforms(self, value):                 # accumulate.ts:178-188
        self.uniforms.set(value)
        self.renderer.ctx.set_uniforms(self.PASS_ID, self.uniforms.tobytes())

    def update(self):                             # accumulate.ts:190-195
        r = self.renderer
        self.setUniforms({"resolution": [r.scaledWidth, r.scaledHeight], "frame": r.frame})

    def render(self, encoder):                    # accumulate.ts:154-176
        encoder.append(capi.SUBMIT_ACCUMULATE)


class FullscreenPass(Pass):
    PASS_ID = capi.PASS_FULLSCREEN

    def __init__(self, renderer):
        super().__init__(renderer)
        self.uniforms = layout.UniformBlock(layout.FULLSCREEN_UNIFORMS)

    def setUniforms(self, value):                 # fullscreen.ts:138-148
        self.uniforms.set(value)
        self.renderer.ctx.set_uniforms(self.PASS_ID, self.uniforms.tobytes())

    def update(self):                             # fullscreen.ts:150-156
        r = self.renderer
        self.setUniforms({"resolution": [r.width, r.height], "aspect": r.aspect,
                          "scalingFactor": r.scalingFactor})

    def render(self, encoder):                    # fullscreen.ts:158-177
        encoder.append(capi.SUBMIT_FULLSCREEN)


class Renderer:
    """renderer.ts:20-468 without the DOM parts (canvas, ResizeObserver)."""

    def __init__(self, ctx, options=None):
        self.ctx = ctx
        # presentLatest False (the default since round 4): the reference's canvas semantics -- every render() that presents gets
        # its own accumulate and fullscreen pass (renderer.ts:379-390).  True (a headless program that only reads the final
        # canvas): the canvas is drawn once per launched batch instead of once per render(); reading it, or a render() after
        # sampling stopped, shows every frame
        self.options = {"enableTimestampQuery": False, "presentLatest": False}
        self.options.update(options or {})
        ctx.set_present_mode(capi.PRESENT_LATEST if self.options["presentLatest"] else capi.PRESENT_EXACT)
        self._width = self._height = 0
        self._frame = 1
        self._scalingFactor = 0.25
        self.frames = 64
        self.samplesPerFrame = 1
        self.status = "idle"
        self.listeners = {}
        self.presentEveryFrame = True      # headless hosts may skip the fullscreen pass
        self._sceneVersion = 0             # scene uploads so far; with the camera and the size: what the feature images depend on
        self._aovKey = None                # ... as they were when all four feature images were last rendered (denoiseGuided)
        self._moments = False              # setMoments: the moments image is kept beside the running mean
        self._despike = False              # the context's firefly pre-pass state, as the last denoiseGuided left it
        self._meanByCount = False          # setMeanByCount: a step's weight comes from the texel's own sample count
        self._trianglesUploaded = 0        # reprojectScene: the triangle count of the last upload (updateScene)
        self._seedOffset = 0               # reproject: frames sampled in earlier views, added to the raytrace pass's `frame` only
        self._validateLeft = 0             # reproject(validate=K): sampled frames still to submit before the held history is merged
        # refit: on scene.needsUpdate with an unchanged triangle count, re-fit the uploaded tree's boxes on the device instead of rebuilding
        # it (RaytracePass._refitScene); False: the reference's rebuild.  refitCostLimit: rebuild after all when the re-fitted tree's SAH
        # figure exceeds the last full build's by more than this factor.  lastRefitCostRatio / lastRefitMs: what the last update did
        # (None: it rebuilt without trying).  While refit is on and a refit is possible, a tree the host supplies in scene.content.nodes is
        # NOT uploaded: the device's topology is kept and content.nodes is REPLACED by the re-fitted records (the host's copy stays the
        # device's); above the limit it is set to None and built for the new positions.  Leave refit off for an update that brings its own tree
        self.refit = False
        self.refitCostLimit = math.inf
        self.lastRefitCostRatio = None
        self.lastRefitMs = None
        self.passes = {"raytrace": RaytracePass(self), "accumulate": AccumulatePass(self),
                       "fullscreen": FullscreenPass(self)}
        if self.options["enableTimestampQuery"]:
            ctx.enable_timing(True)

    # ---- static constructors: renderer.ts:470-533 ----
    @staticmethod
    def diagnostic():
        try:
            n = capi.device_count()
        except capi.Mi3ptError:
            return {"supported": False}
        if n <= 0:
            return {"supported": False}
        return {"supported": True, "info": capi.device_name(0)}

    @staticmethod
    def create(device=0, options=None, tile=None, devices=None):
        """devices = [0, 1, ...]: a device group (mi3pt_create_group) -- the same Renderer on several GPUs of one
        node: tiles dealt in 8-row blocks, the scene replicated, one gather when an image is read."""
        if devices is not None:
            if tile is not None:
                raise ValueError("`devices` and `tile` exclude each other (a device group deals the tiles itself)")
            ctx = capi.Context(devices=list(devices))
        else:
            ctx = capi.Context(device)          # raises "HIP device not found." without a GPU
        if tile is not None:
            ctx.set_tile(*tile)
        return Renderer(ctx, options)

    # ---- sizes: renderer.ts:283-324 ----
    def resize(self, width, height):
        if self._width == width and self._height == height:
            return
        self._width, self._height = int(width), int(height)
        self.ctx.resize(self._width, self._height)
        self._aovKey = None                        # (a resize frees the feature images)
        self.reset()
        self.emit("resize")

    @property
    def scalingFactor(self):
        return self._scalingFactor

    @scalingFactor.setter
    def scalingFactor(self, value):
        self._scalingFactor = value
        self.setUniforms("fullscreen", {"scalingFactor": value})

    width = property(lambda self: self._width)
    height = property(lambda self: self._height)
    scaledWidth = property(lambda self: self._width * self._scalingFactor)
    scaledHeight = property(lambda self: self._height * self._scalingFactor)
    aspect = property(lambda self: self._width / self._height)

    # ---- frame counter: renderer.ts:330-348 ----
    @property
    def hasFramesToSample(self):
        return self._frame <= self.frames

    @property
    def progress(self):
        return self._frame / (self.frames + 1)

    @property
    def frame(self):
        return self._frame

    @frame.setter
    def frame(self, value):
        self._frame = value
        if self._frame > self.frames:
            self.status = "idle"
            self.emit("complete")

    @property
    def timings(self):
        return {k: p.timingAverage for k, p in self.passes.items()}

    def setUniforms(self, which, value):           # renderer.ts:358-360
        self.passes[which].setUniforms(value)

    def update(self, scene, camera):               # renderer.ts:362-364
        self.passes["raytrace"].updateScene(scene, camera)

    def render(self, scene, camera):               # renderer.ts:366-395
        self.update(scene, camera)
        should_sample = self.status == "sampling" and self.hasFramesToSample
        if should_sample:
            self.frame = self._frame + 1
        self.passes["raytrace"].update()
        self.passes["accumulate"].update()
        self.passes["fullscreen"].update()
        encoder = []
        if should_sample:
            self.passes["raytrace"].render(encoder)
            self.emit("progress", self.progress)
        if should_sample:
            self.passes["accumulate"].render(encoder)
        if self.presentEveryFrame:
            self.passes["fullscreen"].render(encoder)
        mask = 0
        for bit in encoder:
            mask |= bit
        if mask:
            self.ctx.submit(mask)                  # queue.submit, renderer.ts:389-390
        if should_sample and self._validateLeft > 0:
            self._validateLeft -= 1
            if self._validateLeft == 0:
                self.mergeHistory()                # (reproject(validate=K): K fresh frames are in; the defaults)
        if should_sample:
            self.passes["raytrace"].updateTimings()
            self.passes["accumulate"].updateTimings()
        if self.presentEveryFrame:
            self.passes["fullscreen"].updateTimings()

    def reset(self):                               # renderer.ts:397-416
        prev = self.status
        self.status = "paused"
        self._validateLeft = 0                     # (the context drops a held history with the mean)
        if self._width:
            self.ctx.reset()
        self.emit("reset")
        self._frame = 1
        self.status = "sampling" if prev == "idle" else prev
        if self.status == "sampling":
            self.emit("start")

    def destroy(self):                             # renderer.ts:418-429
        self.ctx.sync()
        self.ctx.close()

    def start(self):                               # renderer.ts:431-437
        self.status = "idle" if self._frame > self.frames else "sampling"

    def pause(self):                               # renderer.ts:439-444
        if self.status != "paused":
            self.status = "paused"
            self.emit("pause")

    def on(self, event, callback):                 # renderer.ts:446-458
        self.listeners.setdefault(event, []).append(callback)

    def emit(self, event, *args):                  # renderer.ts:460-468
        for cb in self.listeners.get(event, []):
            cb(*args)

    def updateEnvironmentTexture(self, env):       # renderer.ts:132-281
        env = np.asarray(env)
        if env.shape[1] != 1024 or env.shape[0] != 512:
            raise capi.Mi3ptError(1, "Environment texture must be 1024x512 pixels. "
                                     "Please resize the texture and try again.")
        if env.dtype != np.float32:
            raise capi.Mi3ptError(1, "Environment texture must be a floating point texture. "
                                     "Please convert the texture and try again.")
        self.ctx.upload_environment(env)
        self.ctx.upload_environment_cdf(capi.host_env_cdf(env))

    # ---- headless read-back (no counterpart in the reference) ----
    def readOutput(self):
        return self.ctx.read_texture(capi.TEX_OUTPUT)

    def readAccumulation(self):
        return self.ctx.read_texture(capi.TEX_ACCUMULATION)

    def readCanvas(self):
        return self.ctx.read_canvas_rgba8()

    # ---- first-hit feature images (no counterpart in the reference) ----
    def renderAovs(self, names=None):
        """Render the feature images of the first hit (capi.AOV_NAMES: albedo, normal, position, ids; None = all four)
        with the camera and scene of the last update() at the current resolution.  Not a sample frame: `frame`, the
        accumulation image and the counters are untouched."""
        mask = 0
        for name in (capi.AOV_NAMES if names is None else names):
            mask |= 1 << capi.AOV_NAMES.index(name)
        self.passes["raytrace"].update()           # resolution / aspect as render() would send them
        self.ctx.render_aovs(mask)
        if mask == capi.AOV_ALL:
            self._aovKey = self._aovKeyNow()
        elif self._aovKey != self._aovKeyNow():
            self._aovKey = None                    # (some images are of another view now)

    def _aovKeyNow(self):
        u = self.passes["raytrace"].uniforms.tobytes()
        # what a feature image depends on: resolution, aspect, camera position / direction / fov (include/mi3pt.h), scene, size
        return (u[0:12], u[32:44], u[48:64], self._sceneVersion, self._width, self._height)

    # ---- feature-guided de-noise of the running mean (no counterpart in the reference) ----
    VARIANCE_AUTO_FRAMES = 8       # variance="auto": frames in the mean from which the per-pixel variance steers the filter (a choice: DESIGN.md 3)

    def denoiseGuided(self, levels=3, sigmaColor=None, sigmaNormal=0.35, sigmaAlbedo=0.1, sigmaPlane=0.05, present=False, variance=False, young=False,
                      despike=False):
        """Filter the running mean with the edge-avoiding a-trous filter of include/mi3pt.h (mi3pt_denoise_guided); readGuided()
        returns the result, present=True also draws the canvas from it.  variance False: sigmaColor None = 2 / sqrt(frames in the
        mean) -- the noise of the mean falls with the root of its frames.  variance True (MI3PT_GUIDED_VARIANCE; needs
        setMoments(True) before the frames were sampled): the colour weight follows the per-pixel variance of the mean, sigmaColor
        None = 2, readGuidedVariance() returns the filtered variance.  variance "auto": True when the moments image is on and at
        least VARIANCE_AUTO_FRAMES frames are in the mean (below that a variance from so few samples is itself noise), else False.
        young True (MI3PT_GUIDED_YOUNG; variance mode only, a ValueError with variance False): a texel with fewer than four samples --
        disoccluded by reproject(), or any texel right after a reset -- takes its variance from the samples of its 7 x 7 neighbours;
        variance "auto" then chooses the variance mode whenever the moments image is on, from the first frame (with moments off it
        stays the fixed sigma, without the flag).
        despike True (mi3pt_set_guided_despike; any mode): a firefly pre-pass ahead of the filter -- a texel brighter than all 3 x 3
        neighbours of its material and hit flag is scaled down to the brightest of them in the image the filter reads;
        readGuidedDespiked() returns how many were.  The option sets the context's state for this call and leaves it so; the
        default is off.
        The feature images are rendered first unless all four are current for the camera and scene of the last update() at this
        size.  The accumulation image is untouched."""
        frames = max(1, self._frame - 1)
        if variance == "auto":
            variance = self._moments and (bool(young) or frames >= self.VARIANCE_AUTO_FRAMES)
            young = bool(young) and variance
        elif not isinstance(variance, bool):
            raise ValueError("variance must be True, False or 'auto'")
        if young and not variance:
            raise ValueError("young=True needs the variance mode (variance=True or 'auto')")
        self.passes["raytrace"].update()
        if self._aovKey is None or self._aovKey != self._aovKeyNow():
            self.renderAovs()
        if sigmaColor is None:
            sigmaColor = 2.0 if variance else 2.0 / math.sqrt(frames)
        if present:
            self.passes["fullscreen"].update()
        if bool(despike) != self._despike:
            self.ctx.set_guided_despike(bool(despike))
            self._despike = bool(despike)
        self.ctx.denoise_guided(levels, sigmaColor, sigmaNormal, sigmaAlbedo, sigmaPlane,
                                (capi.GUIDED_PRESENT if present else 0) | (capi.GUIDED_VARIANCE if variance else 0) |
                                (capi.GUIDED_YOUNG if young else 0))

    def readGuidedVariance(self):
        """(rows, width) float32: the last level's variance of the last denoiseGuided(variance=True)."""
        return self.ctx.read_guided_variance()

    def readGuidedDespiked(self):
        """The number of texels the pre-pass of the last denoiseGuided(despike=True) clamped."""
        return self.ctx.read_guided_despiked()

    # ---- the moments image: the spread of the frames around the running mean (no counterpart in the reference) ----
    def setMoments(self, enabled=True):
        """Keep (M2.rgb, n) -- Welford's sums around the running mean, include/mi3pt.h: mi3pt_set_moments -- beside the accumulation
        image from now on (the image starts at zero: enable it before sampling starts, or reset()).  The mean is bit-identical."""
        self.ctx.set_moments(bool(enabled))
        self._moments = bool(enabled)
        if not enabled:
            self._meanByCount = False              # (the count is the image's n: the context switches the mode off with it)
            self._validateLeft = 0                 # (... and drops a held history)

    # ---- the mean by count, and the reprojection of the mean across a camera move (no counterpart in the reference) ----
    def setMeanByCount(self, on=True):
        """Weight every accumulate step by the texel's own sample count (include/mi3pt.h: mi3pt_set_mean_by_count) instead of the
        frame counter; enables the moments image itself.  The mean is then the SAMPLE mean: brighter than the default law's by
        (N + 1) / N after N frames, because this host's accumulate `frame` starts at 2 like the reference's."""
        if on and not self._moments:
            self.setMoments(True)
        self.ctx.set_mean_by_count(bool(on))
        self._meanByCount = bool(on)

    def reproject(self, scene, camera, planeTolerance=0.02, normalCosMin=0.9, maxHistory=64, validate=0):
        """What a host calls INSTEAD of reset() when only the camera changed: the running mean and its moments are carried into the
        new view (include/mi3pt.h: mi3pt_reproject), texels the old view did not see restart, and the frame budget starts over.
        Returns True; falls back to reset() and returns False when the scene needs an upload, setMeanByCount is off, nothing has
        been sampled yet, or the context is a rank of a tile split or a device group.  validate = K > 0: the carried mean is held
        (holdHistory) and merged by mergeHistory() with its defaults once render() has submitted K further sampled frames."""
        validate = self._validateFrames(validate)
        ctx = self.ctx
        partial = ctx.group_size != 1 or ctx._tile[1] != 1          # (a device group, or a rank of a tile split as of the last resize)
        if scene.needsUpdate or not self._meanByCount or self._frame <= 1 or not self._width or partial:
            self.reset()
            return False
        self._settleValidation()
        if self._aovKey is None or self._aovKey != self._aovKeyNow():
            self.renderAovs()                      # the old view's features, under the uniforms the mean was sampled with
        self.update(scene, camera)
        ctx.reproject(planeTolerance, normalCosMin, maxHistory)
        self._aovKey = self._aovKeyNow()           # (the call rendered all four images of the new view)
        self._startValidation(validate)
        self.emit("reproject")
        self._seedOffset = (self._seedOffset + self._frame - 1) & 0xFFFFFFFF
        prev = self.status
        self._frame = 1
        self.status = "sampling" if prev == "idle" else prev
        if self.status == "sampling":
            self.emit("start")
        return True

    def reprojectScene(self, scene, camera, planeTolerance=0.02, normalCosMin=0.9, maxHistory=64, maxHistoryMoved=8, validate=0):
        """What a host calls INSTEAD of reset() when scene.needsUpdate is set and the triangle count is unchanged -- an object moved,
        an animation played; the camera may have moved too: texels whose triangle did not move carry as in reproject(), texels whose
        triangle moved follow it back to its old place and carry at most maxHistoryMoved samples (include/mi3pt.h:
        mi3pt_reproject_scene).  Triangle i of the new content must be the surface element triangle i was.  Returns True; falls back
        to reset() and returns False under reproject()'s conditions, when the scene has no content, nothing was uploaded yet or the
        triangle count differs from the last upload.  With scene.needsUpdate clear it is reproject().  validate: as in reproject()."""
        if not scene.needsUpdate:
            return self.reproject(scene, camera, planeTolerance, normalCosMin, maxHistory, validate)
        validate = self._validateFrames(validate)
        ctx = self.ctx
        partial = ctx.group_size != 1 or ctx._tile[1] != 1          # (a device group, or a rank of a tile split as of the last resize)
        count = 0 if scene.content is None else len(scene.content.triangles)
        if not self._meanByCount or self._frame <= 1 or not self._width or partial or count == 0 or count != self._trianglesUploaded:
            self.reset()
            return False
        self._settleValidation()
        if self._aovKey is None or self._aovKey != self._aovKeyNow():
            self.renderAovs()                      # the old view's features of the old scene
        ctx.keep_geometry(True)
        try:
            self.update(scene, camera)             # (uploads: the context hands the old records over instead of freeing them)
            ctx.reproject_scene(planeTolerance, normalCosMin, maxHistory, maxHistoryMoved)
        finally:
            ctx.keep_geometry(False)
        self._aovKey = self._aovKeyNow()           # (the call rendered all four images of the new scene and view)
        self._startValidation(validate)
        self.emit("reproject")
        self._seedOffset = (self._seedOffset + self._frame - 1) & 0xFFFFFFFF
        prev = self.status
        self._frame = 1
        self.status = "sampling" if prev == "idle" else prev
        if self.status == "sampling":
            self.emit("start")
        return True

    # ---- a held history, validated against fresh samples before it is merged (no counterpart in the reference) ----
    def holdHistory(self):
        """Set the running mean and its moments aside and restart the live pair, as reset() would (include/mi3pt.h:
        mi3pt_hold_history); the frame counter, the canvas and the feature images stay.  Needs setMeanByCount(True).  A reset(), a
        resize() and a reproject() drop what is held."""
        self.ctx.hold_history()
        self._validateLeft = 0

    def mergeHistory(self, radius=1, zKeep=2.0, zDrop=4.0):
        """Merge the held history into the mean sampled since holdHistory(): per texel as much of it as a two-sample test of the fresh
        mean against the held one over a (2 * radius + 1)^2 window supports -- all of it up to a z-score of zKeep, none of it from zDrop
        (include/mi3pt.h: mi3pt_merge_history)."""
        self.ctx.merge_history(radius, zKeep, zDrop)
        self._validateLeft = 0

    def _settleValidation(self):
        """a move while a held history waits for its frames: it is merged on what has been sampled so far, not lost"""
        if self._validateLeft > 0:
            self.mergeHistory()

    def _startValidation(self, validate):
        if validate > 0:
            self.holdHistory()
            self._validateLeft = validate

    @staticmethod
    def _validateFrames(validate):
        validate = int(validate)
        if validate < 0:
            raise ValueError("validate must be >= 0")
        return validate

    def readMoments(self):
        """(rows, width, 4) float32: M2.r, M2.g, M2.b, n."""
        return self.ctx.read_moments()

    # ---- sample until converged: the per-tile error estimate of the running mean (no counterpart in the reference) ----
    def estimateConvergence(self, threshold, minFrames=16):
        """Enqueue the error estimate of the mean of every frame rendered so far (include/mi3pt.h: mi3pt_estimate_convergence)."""
        self.ctx.estimate_convergence(threshold, minFrames)

    def readConvergence(self):
        """The summary of the last estimateConvergence: a dict of the nine fields of mi3pt_convergence."""
        return self.ctx.read_convergence()

    def readConvergenceTiles(self):
        """(tiles_y, tiles_x, 4) float32: sum_r, max_r, count, n_min per 8 x 8 tile."""
        return self.ctx.read_convergence_tiles()

    @staticmethod
    def isConverged(summary):
        return summary["tiles"] > 0 and summary["tiles_above"] == 0

    # ---- adaptive sampling: stop sampling the tiles that have converged (include/mi3pt.h: mi3pt_set_sample_mask) ----
    def setSampleMask(self, mask):
        """One value per 8 x 8 tile (tiles_y, tiles_x), non-zero = sampled, zero = frozen: a frozen tile is neither traced nor
        accumulated, its mean and moments keep their bits.  None removes the mask; reset() and resize() drop it."""
        self.ctx.set_sample_mask(mask)

    def readSampleMask(self):
        """(tiles_y, tiles_x) uint8 of 0 / 1; without a mask all 1."""
        return self.ctx.read_sample_mask()

    def freezeConverged(self, guard=1):
        """Freeze the tiles the last estimateConvergence found under its threshold -- with guard 1 only those whose up to eight
        neighbours are under it too, which hides tile borders.  Never thaws.  Returns the number of tiles still sampled."""
        return self.ctx.freeze_converged(guard)

    def renderUntil(self, scene, camera, threshold, minFrames=16, maxFrames=None, checkEvery=None, lookahead=True, adaptive=False,
                    guard=1):
        """render() until every 8 x 8 tile's estimated RMSE of the tone-mapped mean is at most `threshold` and has seen minFrames
        frames, or until maxFrames (None: self.frames, otherwise it becomes self.frames) are in the mean.  The mean is checked every
        checkEvery frames (None: the context's batch capacity, so launches keep one shape).  lookahead: the estimate of a chunk is
        read after the NEXT chunk has been flushed, so the device never idles while the host decides; the run then stops one chunk
        after the estimate that said converged, and those frames stay in the mean.  Without it the run stops at once.  The frame
        count at which it stops is a function of the images alone.  Returns {"converged", "frames", "summary"}; the summary is the
        estimate that stopped the run, or, at the end of the budget, that of the final mean.
        adaptive: after every estimate that is read, freezeConverged(guard) stops sampling the tiles that are done; the run is
        converged when no tile is sampled any more, i.e. every tile was under the threshold at the check that froze it.  With
        lookahead the decision from estimate k is applied after chunk k + 1 has been flushed, so a tile is sampled one chunk longer.
        The summary is then always that of an estimate of the FINAL image, and may show a tile above the threshold although the run
        converged: with lookahead a tile is sampled one chunk beyond the estimate that found it under, and the estimate is not
        monotone in the frames.  Such a tile stays frozen, and with guard 1 it keeps its neighbours sampling (the ring reads frozen
        neighbours too): a run with lookahead and guard 1 can then last to maxFrames -- lookahead=False or guard=0 end it.  The result
        gains "sampled": the tile-frames actually sampled."""
        if not self._moments:
            raise ValueError("renderUntil needs the moments image: setMoments(True) before sampling starts")
        if maxFrames is not None:
            self.frames = int(maxFrames)
        if checkEvery is None:
            checkEvery = self.ctx.batch_capacity()
        checkEvery = max(1, int(checkEvery))
        if adaptive:
            return self._renderUntilAdaptive(scene, camera, threshold, minFrames, checkEvery, lookahead, guard)
        pending = False          # an estimate has been enqueued and not read
        current = False          # `summary` is of the mean as it stands
        summary = None
        while self.status == "sampling" and self.hasFramesToSample:
            for _ in range(min(checkEvery, self.frames - (self._frame - 1))):
                self.render(scene, camera)
            self.ctx.flush()
            if lookahead:
                if pending:
                    summary = self.ctx.read_convergence()      # (the chunk just flushed runs while the host waits)
                    if self.isConverged(summary):
                        return self._converged(summary)
                self.ctx.estimate_convergence(threshold, minFrames)
                pending = True
            else:
                self.ctx.estimate_convergence(threshold, minFrames)
                summary = self.ctx.read_convergence()
                current = True
                if self.isConverged(summary):
                    return self._converged(summary)
        if not current:          # the end of the budget: the result describes the final mean
            if not pending:
                self.ctx.estimate_convergence(threshold, minFrames)
            summary = self.ctx.read_convergence()
        if self.isConverged(summary):
            return self._converged(summary)
        return {"converged": False, "frames": self._frame - 1, "summary": summary}

    def _renderUntilAdaptive(self, scene, camera, threshold, minFrames, checkEvery, lookahead, guard):
        sampling = int(np.count_nonzero(self.ctx.read_sample_mask()))      # tiles the next chunk samples
        sampled = 0              # tile-frames sampled so far
        pending = False          # an estimate has been enqueued and not read
        summary = None           # the summary of the mean as it stands, once read
        done = False
        while self.status == "sampling" and self.hasFramesToSample and not done:
            n = min(checkEvery, self.frames - (self._frame - 1))
            for _ in range(n):
                self.render(scene, camera)
            self.ctx.flush()
            sampled += n * sampling
            summary = None
            if lookahead:
                if pending:
                    self.ctx.read_convergence()                # (the chunk just flushed runs while the host waits)
                    pending = False
                    sampling = self.ctx.freeze_converged(guard)
                    done = sampling == 0
                if not done:
                    self.ctx.estimate_convergence(threshold, minFrames)
                    pending = True
            else:
                self.ctx.estimate_convergence(threshold, minFrames)
                summary = self.ctx.read_convergence()
                sampling = self.ctx.freeze_converged(guard)
                done = sampling == 0
        if summary is None:      # the result describes the final mean
            if not pending:
                self.ctx.estimate_convergence(threshold, minFrames)
            summary = self.ctx.read_convergence()
        out = self._converged(summary) if done else {"converged": False, "frames": self._frame - 1, "summary": summary}
        out["sampled"] = sampled
        return out

    def _converged(self, summary):
        self.emit("converged", summary)
        if self.status != "idle":
            self.status = "idle"
            self.emit("complete")
        return {"converged": True, "frames": self._frame - 1, "summary": summary}

    def readGuided(self):
        """(rows, width, 4) float32: the filtered image of the last denoiseGuided."""
        return self.ctx.read_guided()

    def readAov(self, name):
        """(rows, width, 4) float32 -- int32 for "ids" -- of a feature image rendered by renderAovs."""
        return self.ctx.read_aov(capi.AOV_NAMES.index(name))

    def screenshot(self, path=None):
        """main.ts:351-356 (canvas.toDataURL("image/png")): the presented canvas as PNG bytes."""
        png = encode_png(self.readCanvas())
        if path:
            with open(path, "wb") as f:
                f.write(png)
        return png


def encode_png(rgba8):
    """8-bit RGBA, one IDAT chunk."""
    import struct
    import zlib
    import numpy as np
    img = np.ascontiguousarray(rgba8, np.uint8)
    h, w = img.shape[:2]
    raw = np.zeros((h, w * 4 + 1), np.uint8)
    raw[:, 1:] = img.reshape(h, w * 4)

    def chunk(kind, data):
        body = kind + data
        return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw.tobytes())) + chunk(b"IEND", b""))

