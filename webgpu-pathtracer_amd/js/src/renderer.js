'use strict';
// src/renderer.ts without the DOM: same public API (create / diagnostic / render / update /
// setUniforms / reset / start / pause / resize / destroy / on / emit; frames,
// samplesPerFrame, scalingFactor, status, frame, progress, hasFramesToSample, timings,
// width / height / scaledWidth / scaledHeight / aspect), the GPUDevice replaced by a
// libmi3pt.so context reached through the N-API addon.  canvas / context / format have no
// headless meaning; readOutput / readAccumulation / readCanvas are the read-back a headless
// drop-in needs instead of canvas.toDataURL (src/main.ts:351-356).
const path = require('path');
const { RaytracePass } = require('./passes/raytrace');
const { AccumulatePass } = require('./passes/accumulate');
const { FullscreenPass } = require('./passes/fullscreen');
const { FloatType } = require('./scene');

const TEX_OUTPUT = 0, TEX_ACCUMULATION = 1, TEX_CANVAS = 2;
const AOV_NAMES = ['albedo', 'normal', 'position', 'ids'];      // mi3pt_aov, include/mi3pt.h
const VARIANCE_AUTO_FRAMES = 8;      // denoiseGuided({ variance: 'auto' }): frames in the mean from which the per-pixel variance steers the filter (a choice: DESIGN.md 3)

let nativeModule = null;
function loadNative() {
  if (nativeModule === null) {
    try {
      nativeModule = require(path.join(__dirname, '..', 'mi3pt.node'));
    } catch (err) {
      throw new Error('mi3pt.node / libmi3pt.so not loadable (build with __graft_entry__.build()): ' + err.message);
    }
  }
  return nativeModule;
}

class Renderer {
  constructor(args) {                                   // renderer.ts:47-92
    this.native = args.native;
    this.handle = args.handle;
    // presentEveryFrame: encode the fullscreen pass on every render() like renderer.ts:386 (false: never).
    // presentLatest: false (the default since round 4: the reference's canvas semantics, renderer.ts:379-390) -- every render()
    // gets its own accumulate and fullscreen pass and the canvas is drawn from the mean up to and including this very frame
    // (MI3PT_PRESENT_EXACT; up to 16 such frames share one raytrace launch, every canvas the reference would draw is drawn).
    // true (a headless program that only reads the final canvas): a sample frame that also presents is queued like any other
    // and the canvas is drawn once per launched batch (MI3PT_PRESENT_LATEST: 2.4x the frame rate); reading the canvas, or a
    // render() after sampling has stopped, shows every frame.
    this.options = Object.assign({ enableTimestampQuery: false, verbose: false, presentEveryFrame: true,
      presentLatest: false }, args.options || {});
    this.native.setPresentMode(this.handle, this.options.presentLatest ? 1 : 0);
    this._width = 0;
    this._height = 0;
    this._frame = 1;
    this._scalingFactor = 0.25;
    this.frames = 64;
    this.samplesPerFrame = 1;
    this.status = 'idle';
    this.listeners = new Map();
    this._sceneVersion = 0;      // scene uploads so far; with the camera and the size: what the feature images depend on
    this._aovKey = null;         // ... as they were when all four feature images were last rendered (denoiseGuided)
    this._moments = false;       // setMoments: the moments image is kept beside the running mean
    this._despike = false;       // the context's firefly pre-pass state, as the last denoiseGuided left it
    this._meanByCount = false;   // setMeanByCount: a step's weight comes from the texel's own sample count
    this._trianglesUploaded = 0; // reprojectScene: the triangle count of the last upload (RaytracePass.updateScene)
    this._seedOffset = 0;        // reproject: frames sampled in earlier views, added to the raytrace pass's `frame` only
    this._validateLeft = 0;      // reproject({ validate: K }): sampled frames still to submit before the held history is merged
    // refit: on scene.needsUpdate with an unchanged triangle count, re-fit the uploaded tree's boxes on the device instead of rebuilding
    // it (RaytracePass.refitScene); false: the reference's rebuild.  refitCostLimit: rebuild after all when the re-fitted tree's SAH
    // figure exceeds the last full build's by more than this factor.  lastRefitCostRatio / lastRefitMs: what the last update did
    // (null: it rebuilt without trying)
    this.refit = false;
    this.refitCostLimit = Infinity;
    this.lastRefitCostRatio = null;
    this.lastRefitMs = null;
    this.tile = args.tile || { rank: 0, nranks: 1, blockRows: 8 };
    if (this.options.enableTimestampQuery) this.native.enableTiming(this.handle, 1);
    this.passes = {
      raytrace: new RaytracePass(this),
      accumulate: new AccumulatePass(this),
      fullscreen: new FullscreenPass(this),
    };
  }

  // ---- renderer.ts:470-533
  static async diagnostic() {
    let native;
    try { native = loadNative(); } catch (err) { return { supported: false }; }
    if (native.deviceCount() <= 0) return { supported: false };
    return { supported: true, info: { description: native.deviceName(0), vendor: 'amd', architecture: 'gfx950' } };
  }

  // options.device: one GPU (default 0).  options.devices = [0, 1, ...]: a device group (mi3pt_create_group) -- the
  // image's 8-row blocks are dealt to one member context per listed GPU, the scene is replicated, nothing is
  // exchanged per frame, and reading the accumulation image or the canvas gathers the members' rows with peer
  // copies; the loop below (renderer.ts:366-395) and every read-back stay the same and move whole images.
  static async create(options) {
    const native = loadNative();
    const opts = options || {};
    if (Array.isArray(opts.devices)) {
      if (opts.tile) throw new Error('Renderer.create: `devices` and `tile` exclude each other (a device group deals the tiles itself)');
      const handle = native.createGroup(opts.devices, opts.blockRows || 8);      // throws "HIP device not found."
      const r = new Renderer({ native, handle, options: opts, tile: { rank: 0, nranks: 1, blockRows: opts.blockRows || 8 } });
      r.devices = opts.devices.slice();
      return r;
    }
    const handle = native.create(opts.device || 0);      // throws "HIP device not found." (renderer.ts:514-516)
    const tile = opts.tile || { rank: 0, nranks: 1, blockRows: 8 };
    native.setTile(handle, tile.rank, tile.nranks, tile.blockRows);
    return new Renderer({ native, handle, options: opts, tile });
  }

  // ---- renderer.ts:132-281
  updateEnvironmentTexture(texture) {
    if (texture.image.width !== 1024 || texture.image.height !== 512) {
      throw new Error('Environment texture must be 1024x512 pixels. Please resize the texture and try again.');
    }
    if (texture.type !== FloatType) {
      throw new Error('Environment texture must be a floating point texture. Please convert the texture and try again.');
    }
    const data = texture.image.data;
    this.native.uploadEnvironment(this.handle, data, 1024, 512);
    this.native.uploadEnvironmentCdf(this.handle, this.native.hostEnvCdf(data, 1024, 512), 1024, 512);
  }

  // ---- renderer.ts:283-324
  resize(width, height) {
    if (this._width === width && this._height === height) return;
    this._width = width;
    this._height = height;
    this.native.resize(this.handle, width, height);
    this._aovKey = null;                         // (a resize frees the feature images)
    this.reset();
    this.emit('resize');
  }
  get scalingFactor() { return this._scalingFactor; }
  set scalingFactor(value) {
    this._scalingFactor = value;
    this.setUniforms('fullscreen', { scalingFactor: value });
  }
  get width() { return this._width; }
  get scaledWidth() { return this._width * this._scalingFactor; }
  get height() { return this._height; }
  get scaledHeight() { return this._height * this._scalingFactor; }
  get aspect() { return this._width / this._height; }

  // ---- renderer.ts:330-356
  get hasFramesToSample() { return this._frame <= this.frames; }
  get progress() { return this._frame / (this.frames + 1); }
  get frame() { return this._frame; }
  set frame(value) {
    this._frame = value;
    if (this._frame > this.frames) {
      this.status = 'idle';
      this.emit('complete');
    }
  }
  get timings() {
    return {
      raytrace: this.passes.raytrace.timingAverage,
      accumulate: this.passes.accumulate.timingAverage,
      fullscreen: this.passes.fullscreen.timingAverage,
    };
  }

  setUniforms(pass, value) { this.passes[pass].setUniforms(value); }        // renderer.ts:358-360
  update(scene, camera) { this.passes.raytrace.updateScene(scene, camera); } // renderer.ts:362-364

  render(scene, camera) {                                                    // renderer.ts:366-395
    this.update(scene, camera);
    const shouldSample = this.status === 'sampling' && this.hasFramesToSample;
    if (shouldSample) this.frame++;
    this.passes.raytrace.update();
    this.passes.accumulate.update();
    this.passes.fullscreen.update();
    const commandEncoder = { passes: 0 };
    if (shouldSample) {
      this.passes.raytrace.render(commandEncoder);
      this.emit('progress', this.progress);
    }
    if (shouldSample) this.passes.accumulate.render(commandEncoder);
    if (this.options.presentEveryFrame) this.passes.fullscreen.render(commandEncoder);
    if (commandEncoder.passes) this.native.submit(this.handle, commandEncoder.passes);   // queue.submit
    if (shouldSample && this._validateLeft > 0 && --this._validateLeft === 0) this.mergeHistory();   // (reproject({ validate: K }): K fresh frames are in; the defaults)
    if (shouldSample) this.passes.raytrace.updateTimings();
    if (shouldSample) this.passes.accumulate.updateTimings();
    if (this.options.presentEveryFrame) this.passes.fullscreen.updateTimings();
  }

  reset() {                                                                  // renderer.ts:397-416
    const prevStatus = this.status;
    this.status = 'paused';
    this._validateLeft = 0;                      // (the context drops a held history with the mean)
    if (this._width > 0) this.native.reset(this.handle);
    this.emit('reset');
    this._frame = 1;
    this.status = prevStatus === 'idle' ? 'sampling' : prevStatus;
    if (this.status === 'sampling') this.emit('start');
  }

  async destroy() {                                                          // renderer.ts:418-429
    this.native.sync(this.handle);
    this.native.destroy(this.handle);
  }

  start() { this.status = this._frame > this.frames ? 'idle' : 'sampling'; } // renderer.ts:431-437
  pause() {                                                                  // renderer.ts:439-444
    if (this.status !== 'paused') {
      this.status = 'paused';
      this.emit('pause');
    }
  }
  on(event, callback) {                                                      // renderer.ts:446-458
    if (!this.listeners.has(event)) this.listeners.set(event, []);
    this.listeners.get(event).push(callback);
  }
  emit(event) {                                                              // renderer.ts:460-468
    const args = Array.prototype.slice.call(arguments, 1);
    const list = this.listeners.get(event);
    if (list) list.forEach((callback) => callback.apply(null, args));
  }

  // ---- headless read-back
  get localRows() { return this.native.tileLocalRows(this._height, this.tile.rank, this.tile.nranks, this.tile.blockRows); }
  readOutput() { return this.native.readTexture(this.handle, TEX_OUTPUT, this.localRows * this._width * 4); }
  readAccumulation() { return this.native.readTexture(this.handle, TEX_ACCUMULATION, this.localRows * this._width * 4); }
  readCanvasFloat() { return this.native.readTexture(this.handle, TEX_CANVAS, this._height * this._width * 4); }
  readCanvas() { return this.native.readCanvasRgba8(this.handle, this._height * this._width * 4); }
  counters() { return this.native.getCounters(this.handle); }
  // ---- first-hit feature images (no counterpart in the reference): albedo, normal, position (+ t), ids of the un-jittered camera
  // ray's closest hit, with the camera and scene of the last update() at the current resolution.  Not a sample frame: `frame`, the
  // accumulation image and the counters are untouched.  names: a subset of AOV_NAMES (default: all four).
  renderAovs(names) {
    let mask = 0;
    for (const name of (names || AOV_NAMES)) {
      const k = AOV_NAMES.indexOf(name);
      if (k < 0) throw new Error('renderAovs: unknown feature image "' + name + '" (' + AOV_NAMES.join(', ') + ')');
      mask |= 1 << k;
    }
    this.passes.raytrace.update();               // resolution / aspect as render() would send them
    this.native.renderAovs(this.handle, mask);
    if (mask === 15) this._aovKey = this._aovKeyNow();
    else if (this._aovKey !== this._aovKeyNow()) this._aovKey = null;      // (some images are of another view now)
  }
  // what a feature image depends on: resolution, aspect, camera position / direction / fov (include/mi3pt.h), scene, size
  _aovKeyNow() {
    const u = Buffer.from(this.passes.raytrace.uniforms.bytes.buffer, this.passes.raytrace.uniforms.bytes.byteOffset, 96);
    return [u.toString('hex', 0, 12), u.toString('hex', 32, 44), u.toString('hex', 48, 64), this._sceneVersion, this._width, this._height].join(':');
  }
  // ---- feature-guided de-noise of the running mean (no counterpart in the reference): the edge-avoiding a-trous filter of
  // include/mi3pt.h (mi3pt_denoise_guided).  readGuided() returns the result; present: also draw the canvas from it.  sigmaColor
  // undefined / null: 2 / sqrt(frames in the mean) -- the noise of the mean falls with the root of its frames.  The feature images are
  // rendered first unless all four are current for the camera and scene of the last update() at this size.  The accumulation image is
  // untouched.
  // variance: true (MI3PT_GUIDED_VARIANCE; needs setMoments(true) before the frames were sampled): the colour weight follows the per-pixel
  // variance of the mean, sigmaColor defaults to 2, readGuidedVariance() returns the filtered variance; false (the default): as above;
  // 'auto': true when the moments image is on and at least VARIANCE_AUTO_FRAMES frames are in the mean (below that a variance from so few
  // samples is itself noise), false otherwise.
  // young: true (MI3PT_GUIDED_YOUNG; variance mode only, an Error with variance false): a texel with fewer than four samples -- disoccluded
  // by reproject(), or any texel right after a reset -- takes its variance from the samples of its 7 x 7 neighbours; variance 'auto' then
  // chooses the variance mode whenever the moments image is on, from the first frame (with moments off it stays the fixed sigma, no flag).
  // despike: true (mi3pt_set_guided_despike; any mode): a firefly pre-pass ahead of the filter -- a texel brighter than all 3 x 3 neighbours
  // of its material and hit flag is scaled down to the brightest of them in the image the filter reads; readGuidedDespiked() returns how
  // many were.  The option sets the context's state for this call and leaves it so; the default is off.
  denoiseGuided(options) {
    const o = Object.assign({ levels: 3, sigmaColor: null, sigmaNormal: 0.35, sigmaAlbedo: 0.1, sigmaPlane: 0.05, present: false, variance: false, young: false, despike: false }, options || {});
    const frames = Math.max(1, this._frame - 1);
    if (o.variance !== true && o.variance !== false && o.variance !== 'auto') throw new Error("denoiseGuided: variance must be true, false or 'auto'");
    const variance = o.variance === 'auto' ? this._moments && (!!o.young || frames >= VARIANCE_AUTO_FRAMES) : o.variance;
    const young = !!o.young && (o.variance === 'auto' ? variance : true);
    if (young && !variance) throw new Error("denoiseGuided: young needs the variance mode (variance true or 'auto')");
    this.passes.raytrace.update();
    if (this._aovKey === null || this._aovKey !== this._aovKeyNow()) this.renderAovs();
    const sigmaColor = o.sigmaColor === null || o.sigmaColor === undefined ? (variance ? 2 : 2 / Math.sqrt(frames)) : o.sigmaColor;
    if (o.present) this.passes.fullscreen.update();
    if (!!o.despike !== this._despike) {
      this.native.setGuidedDespike(this.handle, o.despike ? 1 : 0);
      this._despike = !!o.despike;
    }
    this.native.denoiseGuided(this.handle, o.levels, sigmaColor, o.sigmaNormal, o.sigmaAlbedo, o.sigmaPlane, (o.present ? 1 : 0) | (variance ? 2 : 0) | (young ? 4 : 0));
  }
  // localRows x width floats: the last level's variance of the last denoiseGuided({ variance: true })
  readGuidedVariance() { return this.native.readGuidedVariance(this.handle, this.localRows * this._width); }
  // the number of texels the pre-pass of the last denoiseGuided({ despike: true }) clamped
  readGuidedDespiked() { return this.native.readGuidedDespiked(this.handle); }
  // ---- the moments image (no counterpart in the reference): (M2.r, M2.g, M2.b, n) -- Welford's sums around the running mean, include/mi3pt.h:
  // mi3pt_set_moments -- kept beside the accumulation image from now on (it starts at zero: enable it before sampling starts, or reset()).
  // The mean is bit-identical with and without.
  setMoments(enabled) {
    this.native.setMoments(this.handle, enabled ? 1 : 0);
    this._moments = !!enabled;
    if (!enabled) { this._meanByCount = false; this._validateLeft = 0; }   // (the count is the image's n: the context switches the mode off with it and drops a held history)
  }
  // ---- the mean by count and the reprojection of the mean across a camera move (no counterpart in the reference; include/mi3pt.h:
  // mi3pt_set_mean_by_count, mi3pt_reproject).  setMeanByCount(on = true): every accumulate step takes its weight from the texel's own
  // sample count instead of the frame counter; enables the moments image itself.  The mean is then the SAMPLE mean: brighter than the
  // default law's by (N + 1) / N after N frames, because the accumulate `frame` starts at 2 like the reference's.
  setMeanByCount(on) {
    const enabled = on === undefined ? true : !!on;
    if (enabled && !this._moments) this.setMoments(true);
    this.native.setMeanByCount(this.handle, enabled ? 1 : 0);
    this._meanByCount = enabled;
  }
  // reproject(scene, camera, { planeTolerance = 0.02, normalCosMin = 0.9, maxHistory = 64 }): what a host calls INSTEAD of reset() when
  // only the camera changed -- the running mean and its moments are carried into the new view, texels the old view did not see restart,
  // the frame budget starts over.  Returns true; falls back to reset() and returns false when the scene needs an upload, setMeanByCount
  // is off, nothing has been sampled yet, or the context is a rank of a tile split or a device group.  validate: K > 0 (default 0): the
  // carried mean is held (holdHistory) and merged by mergeHistory() with its defaults once render() has submitted K further sampled frames.
  reproject(scene, camera, options) {
    const o = Object.assign({ planeTolerance: 0.02, normalCosMin: 0.9, maxHistory: 64 }, options || {});
    o.validate = Renderer._validateFrames(o.validate);
    const partial = this.tile.nranks !== 1 || Array.isArray(this.devices);
    if (scene.needsUpdate || !this._meanByCount || this._frame <= 1 || !(this._width > 0) || partial) {
      this.reset();
      return false;
    }
    this._settleValidation();
    if (this._aovKey === null || this._aovKey !== this._aovKeyNow()) this.renderAovs();   // the old view's features, under the uniforms the mean was sampled with
    this.update(scene, camera);
    this.native.reproject(this.handle, o.planeTolerance, o.normalCosMin, o.maxHistory);
    this._aovKey = this._aovKeyNow();            // (the call rendered all four images of the new view)
    this._startValidation(o.validate);
    this.emit('reproject');
    this._seedOffset = (this._seedOffset + this._frame - 1) >>> 0;
    const prevStatus = this.status;
    this._frame = 1;
    this.status = prevStatus === 'idle' ? 'sampling' : prevStatus;
    if (this.status === 'sampling') this.emit('start');
    return true;
  }
  // reprojectScene(scene, camera, { planeTolerance = 0.02, normalCosMin = 0.9, maxHistory = 64, maxHistoryMoved = 8 }): what a host calls
  // INSTEAD of reset() when scene.needsUpdate is set and the triangle count is unchanged -- an object moved, an animation played; the camera
  // may have moved too.  Texels whose triangle did not move carry as in reproject(), texels whose triangle moved follow it back to its old
  // place and carry at most maxHistoryMoved samples (include/mi3pt.h: mi3pt_reproject_scene).  Triangle i of the new scene must be the
  // surface element triangle i was: flattenScene's order is fixed, so moving, turning or deforming meshes keeps it.  Returns true; falls
  // back to reset() and returns false under reproject()'s conditions, when the scene has no triangles, nothing was uploaded yet or the
  // triangle count differs from the last upload.  With scene.needsUpdate clear it is reproject().  validate: as in reproject().
  reprojectScene(scene, camera, options) {
    if (!scene.needsUpdate) return this.reproject(scene, camera, options);
    const o = Object.assign({ planeTolerance: 0.02, normalCosMin: 0.9, maxHistory: 64, maxHistoryMoved: 8 }, options || {});
    o.validate = Renderer._validateFrames(o.validate);
    const partial = this.tile.nranks !== 1 || Array.isArray(this.devices);
    const count = RaytracePass.countTriangles(scene);
    if (!this._meanByCount || this._frame <= 1 || !(this._width > 0) || partial || count === 0 || count !== this._trianglesUploaded) {
      this.reset();
      return false;
    }
    this._settleValidation();
    if (this._aovKey === null || this._aovKey !== this._aovKeyNow()) this.renderAovs();   // the old view's features of the old scene
    this.native.keepGeometry(this.handle, 1);
    try {
      this.update(scene, camera);                // (uploads: the context hands the old records over instead of freeing them)
      this.native.reprojectScene(this.handle, o.planeTolerance, o.normalCosMin, o.maxHistory, o.maxHistoryMoved);
    } finally {
      this.native.keepGeometry(this.handle, 0);
    }
    this._aovKey = this._aovKeyNow();            // (the call rendered all four images of the new scene and view)
    this._startValidation(o.validate);
    this.emit('reproject');
    this._seedOffset = (this._seedOffset + this._frame - 1) >>> 0;
    const prevStatus = this.status;
    this._frame = 1;
    this.status = prevStatus === 'idle' ? 'sampling' : prevStatus;
    if (this.status === 'sampling') this.emit('start');
    return true;
  }
  // deviceRefitBvh(): { nodes, ms } -- the boxes of the uploaded tree re-fitted on the device to the triangles as they stand (include/mi3pt.h:
  // mi3pt_device_refit_bvh), ready for native.uploadBvh, and the device time; the context's state does not move.  What update() does by
  // itself under `refit = true`.  hostBvhCost(nodes): the SAH figure of a tree, the summed box areas over the root's (no device).
  deviceRefitBvh() {
    const held = this.passes.raytrace.nodeBytes;
    if (!held) throw new Error('deviceRefitBvh: no scene has been uploaded yet');
    return this.native.deviceRefitBvh(this.handle, held.length / 48);
  }
  hostBvhCost(nodes) { return this.native.hostBvhCost(nodes); }
  // ---- a held history, validated against fresh samples before it is merged (no counterpart in the reference; include/mi3pt.h:
  // mi3pt_hold_history, mi3pt_merge_history).  holdHistory(): the running mean and its moments are set aside and the live pair restarts,
  // as reset() would restart it; the frame counter, the canvas and the feature images stay.  Needs setMeanByCount(true).  A reset(), a
  // resize() and a reproject() drop what is held.  mergeHistory({ radius = 1, zKeep = 2, zDrop = 4 }): per texel as much of the held
  // history as a two-sample test of the fresh mean against the held one over a (2 * radius + 1)^2 window supports is merged into the mean
  // sampled since -- all of it up to a z-score of zKeep, none of it from zDrop.
  holdHistory() {
    this.native.holdHistory(this.handle);
    this._validateLeft = 0;
  }
  mergeHistory(options) {
    const o = Object.assign({ radius: 1, zKeep: 2, zDrop: 4 }, options || {});
    this.native.mergeHistory(this.handle, o.radius, o.zKeep, o.zDrop);
    this._validateLeft = 0;
  }
  // a move while a held history waits for its frames: it is merged on what has been sampled so far, not lost
  _settleValidation() { if (this._validateLeft > 0) this.mergeHistory(); }
  _startValidation(k) {
    if (k > 0) {
      this.holdHistory();
      this._validateLeft = k;
    }
  }
  static _validateFrames(validate) {
    const k = validate === undefined ? 0 : Math.trunc(validate);
    if (!(k >= 0)) throw new Error('validate must be >= 0');
    return k;
  }
  // localRows x width x 4 floats; row 0 = bottom of the picture
  readMoments() { return this.native.readMoments(this.handle, this.localRows * this._width); }
  // ---- sample until converged (no counterpart in the reference): the per-tile error estimate of the running mean, include/mi3pt.h:
  // mi3pt_estimate_convergence.  estimateConvergence enqueues the estimate of the mean of every frame rendered so far; readConvergence
  // returns its summary { tiles, tilesAbove, tilesYoung, tilesNonfinite, texels, worstTile, worstTexel, nMin, threshold } and waits for
  // that estimate only; readConvergenceTiles the map, tilesY x tilesX x 4 floats (sum_r, max_r, count, n_min).
  estimateConvergence(threshold, minFrames) { this.native.estimateConvergence(this.handle, threshold, minFrames === undefined ? 16 : minFrames); }
  readConvergence() { return this.native.readConvergence(this.handle); }
  readConvergenceTiles() {
    return this.native.readConvergenceTiles(this.handle, Math.ceil(this.localRows / 8) * Math.ceil(this._width / 8));
  }
  static isConverged(summary) { return summary.tiles > 0 && summary.tilesAbove === 0; }
  // ---- adaptive sampling (no counterpart in the reference; include/mi3pt.h: mi3pt_set_sample_mask): one byte per 8 x 8 tile, tilesY x tilesX,
  // non-zero = sampled, zero = frozen -- a frozen tile is neither traced nor accumulated, its mean and moments keep their bits.
  // setSampleMask(null) removes the mask; reset() and resize() drop it.  freezeConverged(guard = 1) freezes the tiles the last
  // estimateConvergence found under its threshold (guard 1: and whose up to eight neighbours are, too) and returns the tiles still sampled.
  setSampleMask(mask) {
    this.native.setSampleMask(this.handle, mask === null || mask === undefined ? null : Uint8Array.from(mask, (v) => (v ? 1 : 0)));
  }
  readSampleMask() { return this.native.readSampleMask(this.handle, Math.ceil(this.localRows / 8) * Math.ceil(this._width / 8)); }
  freezeConverged(guard) { return this.native.freezeConverged(this.handle, guard === undefined ? 1 : guard); }
  // render() until every 8 x 8 tile's estimated RMSE of the tone-mapped mean is at most `threshold` and has seen minFrames frames, or
  // until maxFrames (undefined: this.frames, otherwise it becomes this.frames) are in the mean.  The mean is checked every checkEvery
  // frames (undefined: the context's batch capacity, so launches keep one shape).  lookahead (default true): the estimate of a chunk is
  // read after the NEXT chunk has been flushed, so the device never idles while the host decides; the run then stops one chunk after the
  // estimate that said converged, and those frames stay in the mean.  Without it the run stops at once.  The frame count at which it stops
  // is a function of the images alone.  Returns { converged, frames, summary }; the summary is the estimate that stopped the run, or, at
  // the end of the budget, that of the final mean.
  // { adaptive: true, guard: 0 | 1 }: after every estimate that is read, freezeConverged(guard) stops sampling the tiles that are done; the
  // run is converged when no tile is sampled any more, i.e. every tile was under the threshold at the check that froze it.  With lookahead
  // the decision from estimate k is applied after chunk k + 1 has been flushed, so a tile is sampled one chunk longer.  The summary is then
  // always that of an estimate of the FINAL image, and may show a tile above the threshold although the run converged: with lookahead a
  // tile is sampled one chunk beyond the estimate that found it under, and the estimate is not monotone in the frames.  Such a tile stays
  // frozen, and with guard 1 it keeps its neighbours sampling (the ring reads frozen neighbours too): a run with lookahead and guard 1 can
  // then last to maxFrames -- { lookahead: false } or { guard: 0 } end it.  The result gains `sampled`: the tile-frames actually sampled.
  renderUntil(scene, camera, threshold, options) {
    const o = Object.assign({ minFrames: 16, maxFrames: undefined, checkEvery: undefined, lookahead: true, adaptive: false, guard: 1 }, options || {});
    if (!this._moments) throw new Error('renderUntil needs the moments image: setMoments(true) before sampling starts');
    if (o.maxFrames !== undefined && o.maxFrames !== null) this.frames = o.maxFrames;
    const checkEvery = Math.max(1, o.checkEvery === undefined || o.checkEvery === null ? this.native.batchCapacity(this.handle) : o.checkEvery);
    if (o.adaptive) return this._renderUntilAdaptive(scene, camera, threshold, o, checkEvery);
    let pending = false;         // an estimate has been enqueued and not read
    let current = false;         // `summary` is of the mean as it stands
    let summary = null;
    while (this.status === 'sampling' && this.hasFramesToSample) {
      const n = Math.min(checkEvery, this.frames - (this._frame - 1));
      for (let i = 0; i < n; i++) this.render(scene, camera);
      this.native.flush(this.handle);
      if (o.lookahead) {
        if (pending) {
          summary = this.native.readConvergence(this.handle);      // (the chunk just flushed runs while the host waits)
          if (Renderer.isConverged(summary)) return this._converged(summary);
        }
        this.native.estimateConvergence(this.handle, threshold, o.minFrames);
        pending = true;
      } else {
        this.native.estimateConvergence(this.handle, threshold, o.minFrames);
        summary = this.native.readConvergence(this.handle);
        current = true;
        if (Renderer.isConverged(summary)) return this._converged(summary);
      }
    }
    if (!current) {              // the end of the budget: the result describes the final mean
      if (!pending) this.native.estimateConvergence(this.handle, threshold, o.minFrames);
      summary = this.native.readConvergence(this.handle);
    }
    if (Renderer.isConverged(summary)) return this._converged(summary);
    return { converged: false, frames: this._frame - 1, summary };
  }
  _renderUntilAdaptive(scene, camera, threshold, o, checkEvery) {
    let sampling = this.readSampleMask().reduce((n, v) => n + (v ? 1 : 0), 0);      // tiles the next chunk samples
    let sampled = 0;             // tile-frames sampled so far
    let pending = false;         // an estimate has been enqueued and not read
    let summary = null;          // the summary of the mean as it stands, once read
    let done = false;
    while (this.status === 'sampling' && this.hasFramesToSample && !done) {
      const n = Math.min(checkEvery, this.frames - (this._frame - 1));
      for (let i = 0; i < n; i++) this.render(scene, camera);
      this.native.flush(this.handle);
      sampled += n * sampling;
      summary = null;
      if (o.lookahead) {
        if (pending) {
          this.native.readConvergence(this.handle);      // (the chunk just flushed runs while the host waits)
          pending = false;
          sampling = this.native.freezeConverged(this.handle, o.guard);
          done = sampling === 0;
        }
        if (!done) {
          this.native.estimateConvergence(this.handle, threshold, o.minFrames);
          pending = true;
        }
      } else {
        this.native.estimateConvergence(this.handle, threshold, o.minFrames);
        summary = this.native.readConvergence(this.handle);
        sampling = this.native.freezeConverged(this.handle, o.guard);
        done = sampling === 0;
      }
    }
    if (summary === null) {      // the result describes the final mean
      if (!pending) this.native.estimateConvergence(this.handle, threshold, o.minFrames);
      summary = this.native.readConvergence(this.handle);
    }
    const out = done ? this._converged(summary) : { converged: false, frames: this._frame - 1, summary };
    out.sampled = sampled;
    return out;
  }
  _converged(summary) {
    this.emit('converged', summary);
    if (this.status !== 'idle') {
      this.status = 'idle';
      this.emit('complete');
    }
    return { converged: true, frames: this._frame - 1, summary };
  }
  // localRows x width x 4 floats: the filtered image of the last denoiseGuided; row 0 = bottom of the picture
  readGuided() { return this.native.readGuided(this.handle, this.localRows * this._width); }
  // localRows x width x 4: Float32Array, Int32Array for 'ids' (triangle, material, hit, 0); row 0 = bottom of the picture
  readAov(name) {
    const k = AOV_NAMES.indexOf(name);
    if (k < 0) throw new Error('readAov: unknown feature image "' + name + '" (' + AOV_NAMES.join(', ') + ')');
    return this.native.readAov(this.handle, k, this.localRows * this._width);
  }
  // main.ts:351-356 (canvas.toDataURL("image/png")): the presented canvas as a PNG file
  screenshot(file) {
    const png = encodePNG(this.readCanvas(), this._width, this._height);
    if (file) require('fs').writeFileSync(file, png);
    return png;
  }
  // write the HDR accumulation image back (checkpoint/resume; a gathered multi-GPU image)
  writeAccumulation(data) { this.native.writeTexture(this.handle, TEX_ACCUMULATION, data); }
  // launch queued sample frames now without waiting for them (render() only queues them)
  flush() { this.native.flush(this.handle); }
  // queue.onSubmittedWorkDone() (renderer.ts:420), blocking: everything rendered so far has finished
  sync() { this.native.sync(this.handle); }
  // run the reference's dormant environment importance sampling (raytrace.wgsl:398-404 un-commented)
  setEnvironmentSampling(enabled) { this.native.setEnvSampling(this.handle, enabled ? 1 : 0); this.reset(); }
  raytraceLaunchStats(reset) { return this.native.raytraceLaunchStats(this.handle, reset ? 1 : 0); }
}

// Minimal PNG writer (8-bit RGBA, one IDAT, zlib from Node): what canvas.toDataURL("image/png") holds
function encodePNG(rgba, width, height) {
  const zlib = require('zlib');
  const crcTable = [];
  for (let n = 0; n < 256; n++) {
    let c = n;
    for (let k = 0; k < 8; k++) c = c & 1 ? 0xedb88320 ^ (c >>> 1) : c >>> 1;
    crcTable[n] = c >>> 0;
  }
  const crc32 = (buf) => {
    let c = 0xffffffff;
    for (let i = 0; i < buf.length; i++) c = crcTable[(c ^ buf[i]) & 0xff] ^ (c >>> 8);
    return (c ^ 0xffffffff) >>> 0;
  };
  const chunk = (type, data) => {
    const body = Buffer.concat([Buffer.from(type, 'ascii'), data]);
    const out = Buffer.alloc(8 + data.length + 4);
    out.writeUInt32BE(data.length, 0);
    body.copy(out, 4);
    out.writeUInt32BE(crc32(body), 8 + data.length);
    return out;
  };
  const ihdr = Buffer.alloc(13);
  ihdr.writeUInt32BE(width, 0);
  ihdr.writeUInt32BE(height, 4);
  ihdr[8] = 8; ihdr[9] = 6; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
  const raw = Buffer.alloc((width * 4 + 1) * height);
  for (let y = 0; y < height; y++) {
    raw[y * (width * 4 + 1)] = 0;
    Buffer.from(rgba.buffer, rgba.byteOffset + y * width * 4, width * 4).copy(raw, y * (width * 4 + 1) + 1);
  }
  return Buffer.concat([Buffer.from([0x89, 0x50, 0x4e, 0x47, 0x0d, 0x0a, 0x1a, 0x0a]), chunk('IHDR', ihdr),
    chunk('IDAT', zlib.deflateSync(raw)), chunk('IEND', Buffer.alloc(0))]);
}

module.exports = { Renderer, loadNative, encodePNG, AOV_NAMES, VARIANCE_AUTO_FRAMES };
