// Typed surface of the Node host (hand-written: there is no tsc in the build image).
// Names and semantics follow umar-ahmed/webgpu-pathtracer src/renderer.ts, src/passes/*.ts
// and src/scene.ts; browser-only members (canvas, context, format, device) are absent and
// read-back methods are added for headless use.

export class Vector3 {
  x: number; y: number; z: number;
  constructor(x?: number, y?: number, z?: number);
  set(x: number, y: number, z: number): this;
  copy(v: Vector3): this;
  toArray(): [number, number, number];
  normalize(): this;
}
export class Quaternion { x: number; y: number; z: number; w: number; }
export class Matrix4 { elements: number[]; }
export class Matrix3 { elements: number[]; getNormalMatrix(m: Matrix4): this; }
export class Color { r: number; g: number; b: number; set(r: number, g: number, b: number): this; toArray(): number[]; }

export const FloatType: number;
export class BufferAttribute { array: Float32Array | Uint32Array; itemSize: number; count: number; }
export class BufferGeometry {
  setIndex(indices: number[] | Uint32Array): this;
  getIndex(): BufferAttribute | null;
  setAttribute(name: string, attr: BufferAttribute): this;
  getAttribute(name: string): BufferAttribute;
}
export class PlaneGeometry extends BufferGeometry { constructor(width?: number, height?: number, widthSegments?: number, heightSegments?: number); }
export class BoxGeometry extends BufferGeometry { constructor(width?: number, height?: number, depth?: number, ws?: number, hs?: number, ds?: number); }
export class SphereGeometry extends BufferGeometry { constructor(radius?: number, widthSegments?: number, heightSegments?: number); }
export class Object3D {
  position: Vector3; quaternion: Quaternion; scale: Vector3; visible: boolean;
  matrix: Matrix4; matrixWorld: Matrix4; children: Object3D[];
  add(o: Object3D): this; remove(o: Object3D): this; clear(): this;
  rotateX(a: number): this; rotateY(a: number): this; rotateZ(a: number): this;
  updateMatrixWorld(force?: boolean): void;
  traverse(cb: (o: Object3D) => void): void;
}
export class Mesh extends Object3D { geometry: BufferGeometry; material: RaytracingMaterial; constructor(g: BufferGeometry, m: RaytracingMaterial); }
export class DataTexture { image: { data: Float32Array; width: number; height: number }; type: number; constructor(data: Float32Array, width: number, height: number, type?: number); }

/** src/scene.ts:3-5 */
export class RaytracingScene extends Object3D { needsUpdate: boolean; environment: DataTexture | null; background: DataTexture | null; }
/** src/scene.ts:7-10 */
export class RaytracingCamera extends Object3D {
  fov: number; focalDistance: number; aperture: number;
  constructor(fov?: number, aspect?: number, near?: number, far?: number);
  lookAt(x: number | Vector3, y?: number, z?: number): this;
  getWorldPosition(target: Vector3): Vector3;
  getWorldDirection(target: Vector3): Vector3;
}
/** src/scene.ts:12-14 */
export class RaytracingMaterial {
  color: Color; specularColor: Color; emissive: Color;
  roughness: number; metalness: number; emissiveIntensity: number;
}

export class RollingAverage { addSample(v: number): void; readonly value: number; }

/** src/passes/pass.ts:4-27 */
export abstract class Pass {
  timingAverage: RollingAverage;
  constructor(renderer: Renderer);
  abstract render(commandEncoder: { passes: number }): void;
  abstract update(): void;
  updateTimings(): void;
}
export class RaytracePass extends Pass {
  setUniforms(value: object): void; update(): void; render(e: { passes: number }): void;
  updateScene(scene: RaytracingScene, camera: RaytracingCamera): void;
  stats: { Triangles: number; Materials: number; 'BVH Nodes': number };
}
export class AccumulatePass extends Pass { setUniforms(value: object): void; update(): void; render(e: { passes: number }): void; }
export class FullscreenPass extends Pass { setUniforms(value: object): void; update(): void; render(e: { passes: number }): void; }

export type RendererEventType = 'start' | 'pause' | 'reset' | 'progress' | 'complete' | 'resize' | 'converged' | 'reproject';
export interface RendererOptions {
  device?: number;
  enableTimestampQuery?: boolean;
  presentEveryFrame?: boolean;
  /** default false: the reference's canvas semantics (a fullscreen pass per render()); true: draw the canvas once per launched batch (headless programs that only read the final canvas) */
  presentLatest?: boolean;
  verbose?: boolean;
  builderThreads?: number;
  /** build the tree on the GPU instead of the reference's SAH tree on the host (same closest hits).  true / 'lbvh': a linear BVH (fast on huge
   *  meshes, more box tests per ray); 'ploc': locally-ordered clustering (include/mi3pt.h: mi3pt_device_build_bvh_ex), trees of the SAH
   *  class.  Under `refit`, also the rebuild above refitCostLimit (lastRefitMs then reports that build).  Default: off */
  deviceBvh?: boolean | 'lbvh' | 'ploc';
  /** 'ploc': how many positions to either side a cluster looks for its partner, 1 .. 64 (default 16) */
  deviceBvhRadius?: number;
  /** multi-GPU tile split: this process renders the blockRows-row blocks dealt to `rank`, round after round, BACK AND FORTH
   *  (rank r owns block r of even rounds and block nranks - 1 - r of odd ones: include/mi3pt.h, mi3pt_set_tile).  Use
   *  native.tileGlobalRow(localRow, rank, nranks, blockRows) / native.tileOwner(y, nranks, blockRows) to de-interleave
   *  gathered rows -- never a copy of the formula (it changed with ABI 3) */
  tile?: { rank: number; nranks: number; blockRows: number };
  /** a device group inside this one process (mi3pt_create_group): the image's blockRows-row blocks are dealt to one
   *  member context per listed GPU; render(), the read-backs and the events are unchanged and move whole images */
  devices?: number[];
  blockRows?: number;
}
/** src/renderer.ts:20-468 */
export class Renderer {
  frames: number; samplesPerFrame: number; scalingFactor: number;
  status: 'idle' | 'sampling' | 'paused';
  readonly frame: number; readonly progress: number; readonly hasFramesToSample: boolean;
  readonly width: number; readonly height: number; readonly scaledWidth: number; readonly scaledHeight: number; readonly aspect: number;
  readonly timings: { raytrace: RollingAverage; accumulate: RollingAverage; fullscreen: RollingAverage };
  static diagnostic(): Promise<{ supported: false } | { supported: true; info: { description: string } }>;
  static create(options?: RendererOptions): Promise<Renderer>;
  render(scene: RaytracingScene, camera: RaytracingCamera): void;
  update(scene: RaytracingScene, camera: RaytracingCamera): void;
  setUniforms(pass: 'raytrace' | 'accumulate' | 'fullscreen', value: object): void;
  updateEnvironmentTexture(texture: DataTexture): void;
  resize(width: number, height: number): void;
  reset(): void; start(): void; pause(): void; destroy(): Promise<void>;
  on(event: RendererEventType, callback: (...args: any[]) => void): void;
  emit(event: RendererEventType, ...args: any[]): void;
  /** headless read-back: RGBA float, row 0 = bottom of the picture */
  readOutput(): Float32Array; readAccumulation(): Float32Array;
  /** the fullscreen pass's target, row 0 = top */
  readCanvasFloat(): Float32Array; readCanvas(): Uint8Array;
  /** first-hit feature images of the un-jittered camera rays (camera and scene of the last update()); default: all four */
  renderAovs(names?: Array<'albedo' | 'normal' | 'position' | 'ids'>): void;
  /** localRows x width x 4, row 0 = bottom: albedo rgb 1 | normal xyz 0 | position xyz t | (Int32Array) triangle, material, hit, 0 */
  readAov(name: 'albedo' | 'normal' | 'position'): Float32Array;
  readAov(name: 'ids'): Int32Array;
  /** feature-guided a-trous de-noise of the running mean (include/mi3pt.h: mi3pt_denoise_guided); renders the feature images itself when
   *  none are current.  sigmaColor null: 2 / sqrt(frames in the mean).  present: also draw the canvas from the filtered image.
   *  variance true (MI3PT_GUIDED_VARIANCE; needs setMoments(true)): the colour weight follows the per-pixel variance of the mean and
   *  sigmaColor null is 2; 'auto': true when the moments image is on and at least VARIANCE_AUTO_FRAMES frames are in the mean; default false.
   *  young true (MI3PT_GUIDED_YOUNG; variance mode only): a texel with fewer than four samples takes its variance from the samples of its
   *  7 x 7 neighbours, and 'auto' chooses the variance mode whenever the moments image is on, from the first frame; default false.
   *  despike true (mi3pt_set_guided_despike; any mode): a firefly pre-pass ahead of the filter scales a texel brighter than all 3 x 3
   *  neighbours of its material and hit flag down to the brightest of them, in the image the filter reads; the option sets the context's
   *  state for this call and leaves it so; default false */
  denoiseGuided(options?: { levels?: number; sigmaColor?: number | null; sigmaNormal?: number; sigmaAlbedo?: number; sigmaPlane?: number;
    present?: boolean; variance?: boolean | 'auto'; young?: boolean; despike?: boolean }): void;
  /** localRows x width x 4, row 0 = bottom: the filtered image of the last denoiseGuided */
  readGuided(): Float32Array;
  /** localRows x width, row 0 = bottom: the last level's variance of the last denoiseGuided({ variance: true }) */
  readGuidedVariance(): Float32Array;
  /** the number of texels the pre-pass of the last denoiseGuided({ despike: true }) clamped */
  readGuidedDespiked(): number;
  /** keep the moments image (M2.r, M2.g, M2.b, n: Welford's sums around the running mean; include/mi3pt.h: mi3pt_set_moments) beside the
   *  accumulation image from now on; it starts at zero.  The mean is bit-identical with and without.  Default off */
  setMoments(enabled: boolean): void;
  /** localRows x width x 4, row 0 = bottom */
  readMoments(): Float32Array;
  /** enqueue the per-tile error estimate of the mean of every frame rendered so far (include/mi3pt.h: mi3pt_estimate_convergence);
   *  needs setMoments(true).  minFrames defaults to 16 */
  estimateConvergence(threshold: number, minFrames?: number): void;
  /** the summary of the last estimateConvergence; waits for that estimate only.  Converged: tiles > 0 && tilesAbove === 0 */
  readConvergence(): ConvergenceSummary;
  /** tilesY x tilesX x 4: (sum_r, max_r, count, n_min) per 8 x 8 tile, row 0 = bottom */
  readConvergenceTiles(): Float32Array;
  static isConverged(summary: ConvergenceSummary): boolean;
  /** render() until every tile's estimated RMSE of the tone-mapped mean is at most `threshold` or maxFrames (default: frames) are in the
   *  mean; checked every checkEvery frames (default: the batch capacity).  lookahead (default true): the estimate is read one chunk late,
   *  so the device never idles.  Emits 'converged' with the summary, then 'complete' */
  renderUntil(scene: RaytracingScene, camera: RaytracingCamera, threshold: number,
    options?: { minFrames?: number; maxFrames?: number; checkEvery?: number; lookahead?: boolean; adaptive?: boolean; guard?: 0 | 1 }): { converged: boolean; frames: number; summary: ConvergenceSummary; sampled?: number };
  /** adaptive sampling: one byte per 8 x 8 tile (tilesY x tilesX), non-zero = sampled, zero = frozen; null removes the mask (include/mi3pt.h: mi3pt_set_sample_mask) */
  setSampleMask(mask: ArrayLike<number> | null): void;
  readSampleMask(): Uint8Array;
  /** freeze the tiles the last estimateConvergence found under its threshold; returns the tiles still sampled */
  freezeConverged(guard?: 0 | 1): number;
  /** weight every accumulate step by the texel's own sample count instead of the frame counter (include/mi3pt.h: mi3pt_set_mean_by_count);
   *  enables the moments image itself.  The mean is then the sample mean: brighter than the default law's by (N + 1) / N after N frames.
   *  Default off; `on` defaults to true */
  setMeanByCount(on?: boolean): void;
  /** instead of reset() when only the camera changed: carries the running mean and its moments into the new view (include/mi3pt.h:
   *  mi3pt_reproject), texels the old view did not see restart, the frame budget starts over; emits 'reproject'.  Returns true; falls back
   *  to reset() and returns false when the scene needs an upload, setMeanByCount is off, nothing has been sampled yet, or the renderer is
   *  a rank of a tile split or a device group.  Defaults: planeTolerance 0.02, normalCosMin 0.9, maxHistory 64 */
  reproject(scene: RaytracingScene, camera: RaytracingCamera, options?: { planeTolerance?: number; normalCosMin?: number; maxHistory?: number }): boolean;
  /** ... with validate: K > 0 the carried mean is held (holdHistory) and merged by mergeHistory() with its defaults once render() has
   *  submitted K further sampled frames; 0, the default, merges at once as above */
  reproject(scene: RaytracingScene, camera: RaytracingCamera, options: { planeTolerance?: number; normalCosMin?: number; maxHistory?: number; validate?: number }): boolean;
  /** instead of reset() when scene.needsUpdate is set and the triangle count is unchanged (an object moved, an animation played; the camera
   *  may have moved too): texels whose triangle did not move carry as in reproject(), texels whose triangle moved follow it back to its old
   *  place and carry at most maxHistoryMoved samples (include/mi3pt.h: mi3pt_reproject_scene); emits 'reproject'.  Triangle i of the new
   *  scene must be the surface element triangle i was.  Returns true; falls back to reset() and returns false under reproject()'s conditions,
   *  when the scene has no triangles, nothing was uploaded yet or the triangle count differs from the last upload.  With scene.needsUpdate
   *  clear it is reproject().  Defaults: planeTolerance 0.02, normalCosMin 0.9, maxHistory 64, maxHistoryMoved 8 */
  reprojectScene(scene: RaytracingScene, camera: RaytracingCamera, options?: { planeTolerance?: number; normalCosMin?: number; maxHistory?: number; maxHistoryMoved?: number }): boolean;
  /** ... validate: as in reproject() */
  reprojectScene(scene: RaytracingScene, camera: RaytracingCamera, options: { planeTolerance?: number; normalCosMin?: number; maxHistory?: number; maxHistoryMoved?: number; validate?: number }): boolean;
  /** opt-in: on scene.needsUpdate with the triangle count of the last upload, re-fit the boxes of the uploaded tree on the device
   *  (include/mi3pt.h: mi3pt_device_refit_bvh: the exact boxes of the old topology) instead of rebuilding the SAH tree on the host; the
   *  triangles are uploaded first, then the re-fitted records.  reprojectScene() goes through the same path.  Default false */
  refit: boolean;
  /** rebuild after all when the re-fitted tree's hostBvhCost exceeds that of the last full build by more than this factor.  Default Infinity */
  refitCostLimit: number;
  /** what the last scene update did: cost of the re-fitted tree over the last full build's, and the device time of the refit; null when
   *  the update rebuilt without trying (refit off, first upload, another triangle count) */
  readonly lastRefitCostRatio: number | null;
  readonly lastRefitMs: number | null;
  /** the boxes of the uploaded tree re-fitted on the device to the triangles as they stand, as 48-byte records, and the device time */
  deviceRefitBvh(): { nodes: Buffer; ms: number };
  /** mi3pt_host_bvh_cost: the summed box areas of every 48-byte record over the root's (no device) */
  hostBvhCost(nodes: Uint8Array): number;
  /** set the running mean and its moments aside and restart the live pair as reset() would (include/mi3pt.h: mi3pt_hold_history); the frame
   *  counter, the canvas and the feature images stay.  Needs setMeanByCount(true).  A reset(), a resize() and a reproject() drop what is held */
  holdHistory(): void;
  /** merge the held history into the mean sampled since holdHistory(): per texel as much of it as a two-sample test of the fresh mean against
   *  the held one over a (2 * radius + 1)^2 window supports -- all of it up to a z-score of zKeep, none of it from zDrop (include/mi3pt.h:
   *  mi3pt_merge_history).  Defaults: radius 1, zKeep 2, zDrop 4 */
  mergeHistory(options?: { radius?: number; zKeep?: number; zDrop?: number }): void;
  counters(): { rays: number; boxTests: number; triTests: number; hits: number; misses: number; stackOverflows: number; pixels: number };
  /** src/main.ts:351-356: the presented canvas as PNG bytes (written to `file` when given) */
  screenshot(file?: string): Buffer;
  /** write the HDR accumulation image back (checkpoint / resume, gathered multi-GPU image) */
  writeAccumulation(data: Float32Array): void;
  /** launch the sample frames render() has queued, without waiting for them */
  flush(): void;
  raytraceLaunchStats(reset?: boolean): { totalMs: number; launches: number; frames: number };
  /** the reference's dormant environment importance sampling (raytrace.wgsl:398-404 un-commented); default off */
  setEnvironmentSampling(enabled: boolean): void;
}

/** mi3pt_convergence */
export interface ConvergenceSummary {
  tiles: number; tilesAbove: number; tilesYoung: number; tilesNonfinite: number; texels: number;
  worstTile: number; worstTexel: number; nMin: number; threshold: number;
}

/** src/main.ts:251-266 -- .glb / .gltf (no Draco) to a node hierarchy of indexed meshes */
export class GLTFLoader {
  parse(data: ArrayBuffer | Uint8Array | string | object, baseDir?: string): { scene: Object3D; scenes: Object3D[]; asset: object };
  load(file: string): { scene: Object3D; scenes: Object3D[]; asset: object };
}
export class OBJLoader { parse(text: string): Object3D; load(file: string): Object3D; }
/** src/main.ts:41-46 -- Radiance .hdr to RGBA float texels (FloatType) */
export class RGBELoader { setDataType(type: number): this; parse(buffer: ArrayBuffer | Uint8Array): DataTexture; load(file: string): DataTexture; }
/** the `white` material of src/main.ts:49-53 */
export function whiteMaterial(): RaytracingMaterial;
/** src/main.ts:268-279: position (0, 0.5, 0), uniform scale 1 / max(bounds.max), one material */
export function placeModel(model: Object3D, material?: RaytracingMaterial): Object3D;
export function boundsOfObject(object: Object3D): { min: Vector3; max: Vector3 };
export function encodePNG(rgba: Uint8Array, width: number, height: number): Buffer;
export const AOV_NAMES: Array<'albedo' | 'normal' | 'position' | 'ids'>;
/** denoiseGuided({ variance: 'auto' }) uses the variance mode from this many frames in the mean on */
export const VARIANCE_AUTO_FRAMES: number;
