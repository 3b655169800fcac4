'use strict';
// src/passes/raytrace.ts -- uniforms, scene flattening and upload.  BVH construction
// (buildBVH / buildBVHRecursive / flattenBVH, :540-694) is delegated to the native builder
// (mi3pt_host_build_bvh_f64), which produces the identical tree from the same doubles.
const { Pass } = require('./pass');
const { StructuredView } = require('../layout');
const { Vector3, Matrix3 } = require('../math3');
const { Mesh, RaytracingMaterial } = require('../scene');

const PASS_RAYTRACE = 0, SUBMIT_RAYTRACE = 1;

class RaytracePass extends Pass {
  constructor(renderer) {
    super(renderer);
    this.passId = PASS_RAYTRACE;
    this.uniforms = new StructuredView('RaytraceUniforms');
    this.stats = { Triangles: 0, Materials: 0, 'BVH Nodes': 0 };
  }

  setUniforms(value) {                       // raytrace.ts:359-369
    this.uniforms.set(value);
    this.renderer.native.setUniforms(this.renderer.handle, this.passId, this.uniforms.bytes);
  }

  update() {                                 // raytrace.ts:371-378
    this.setUniforms({
      resolution: [this.renderer.scaledWidth, this.renderer.scaledHeight],
      aspect: this.renderer.aspect,
      // (_seedOffset: 0 unless reproject() was ever called -- a new view's samples must not replay the old view's random sequences)
      frame: (this.renderer.frame + (this.renderer._seedOffset || 0)) >>> 0,
      samplesPerFrame: this.renderer.samplesPerFrame,
    });
  }

  // raytrace.ts:406-502: indexed meshes -> world-space triangles + de-duplicated materials
  static flattenScene(scene) {
    scene.updateMatrixWorld(true);
    const meshes = [];
    scene.traverse((object) => {
      if (object instanceof Mesh && object.visible && object.material instanceof RaytracingMaterial) {
        meshes.push(object);
      }
    });
    const triangles = [];
    const materials = [];
    for (const mesh of meshes) {
      const indices = mesh.geometry.getIndex();
      const positions = mesh.geometry.getAttribute('position');
      const normals = mesh.geometry.getAttribute('normal');
      if (!indices) {
        console.warn('Mesh does not have indices');      // raytrace.ts:499-501
        continue;
      }
      const normalMatrix = new Matrix3().getNormalMatrix(mesh.matrixWorld);
      for (let i = 0; i < indices.array.length; i += 3) {
        const tri = { p: [], n: [] };
        for (let k = 0; k < 3; k++) {
          const vi = indices.array[i + k];
          tri.p.push(new Vector3().fromBufferAttribute(positions, vi).applyMatrix4(mesh.matrixWorld));
          tri.n.push(new Vector3().fromBufferAttribute(normals, vi).applyMatrix3(normalMatrix).normalize());
        }
        let materialIndex = materials.indexOf(mesh.material);
        if (materialIndex === -1) {
          materialIndex = materials.length;
          materials.push(mesh.material);
        }
        tri.materialIndex = materialIndex;
        triangles.push(tri);
      }
    }
    return { triangles, materials };
  }

  // how many triangles flattenScene would make of the scene, without making them (Renderer.reprojectScene compares it with the last upload's)
  static countTriangles(scene) {
    let count = 0;
    scene.traverse((object) => {
      if (object instanceof Mesh && object.visible && object.material instanceof RaytracingMaterial) {
        const indices = object.geometry.getIndex();
        if (indices) count += Math.ceil(indices.array.length / 3);
      }
    });
    return count;
  }

  // raytrace.ts:104-121 / :138-160: structured views -> bytes
  static packScene(flat) {
    const { triangles, materials } = flat;
    const triView = new StructuredView('Triangle', Math.max(triangles.length, 1));
    const positions = new Float64Array(triangles.length * 9);
    for (let i = 0; i < triangles.length; i++) {
      const t = triangles[i];
      triView.set(i, {
        aPosition: t.p[0].toArray(), bPosition: t.p[1].toArray(), cPosition: t.p[2].toArray(),
        aNormal: t.n[0].toArray(), bNormal: t.n[1].toArray(), cNormal: t.n[2].toArray(),
        materialIndex: t.materialIndex,
      });
      for (let k = 0; k < 3; k++) {
        positions[9 * i + 3 * k] = t.p[k].x;
        positions[9 * i + 3 * k + 1] = t.p[k].y;
        positions[9 * i + 3 * k + 2] = t.p[k].z;
      }
    }
    const matView = new StructuredView('Material', Math.max(materials.length, 1));
    for (let i = 0; i < materials.length; i++) {
      const m = materials[i];
      matView.set(i, {
        color: m.color.toArray(), specularColor: m.specularColor.toArray(), roughness: m.roughness,
        metalness: m.metalness, emissionColor: m.emissive.toArray(), emissionStrength: m.emissiveIntensity,
      });
    }
    return { triangleBytes: triView.bytes, materialBytes: matView.bytes, positions };
  }

  // options.deviceBvh / deviceBvhRadius -> null (the default: the host's SAH build), or the arguments of native.deviceBuildBvhEx
  static deviceBuilder(options) {
    const which = options.deviceBvh;
    if (which === undefined || which === null || which === false) return null;
    const method = which === true ? 'lbvh' : which;
    if (method !== 'lbvh' && method !== 'ploc') throw new Error("options.deviceBvh: expected true, 'lbvh' or 'ploc', got " + String(which));
    const radius = options.deviceBvhRadius === undefined ? 16 : options.deviceBvhRadius;
    if (!Number.isInteger(radius) || radius < 1 || radius > 64) throw new Error('options.deviceBvhRadius: expected an integer 1 .. 64, got ' + String(radius));
    return { method: method === 'ploc' ? 1 : 0, radius, maxSearchIterations: 1024 };
  }

  updateScene(scene, camera) {               // raytrace.ts:380-533
    this.setUniforms({
      camera: {
        position: camera.getWorldPosition(new Vector3()).toArray(),
        direction: camera.getWorldDirection(new Vector3()).toArray(),
        fov: camera.fov,
        focalDistance: camera.focalDistance,
        aperture: camera.aperture,
      },
    });
    if (!scene.needsUpdate) return;

    const environment = scene.environment;
    if (environment) this.renderer.updateEnvironmentTexture(environment);

    const flat = RaytracePass.flattenScene(scene);
    if (flat.triangles.length === 0) throw new Error('Input nodes array is empty');    // raytrace.ts:563-565
    const packed = RaytracePass.packScene(flat);
    const native = this.renderer.native, handle = this.renderer.handle;
    const builder = RaytracePass.deviceBuilder(this.renderer.options);
    let nodeBytes = this.renderer.refit ? this.refitScene(packed, flat.triangles.length) : null;
    if (nodeBytes) {
      // (refitScene uploaded the triangles and the tree)
    } else if (builder) {
      // options.deviceBvh: a tree built on the GPU from the uploaded triangles instead of the reference's SAH tree -- same closest hits.
      // true / 'lbvh': the linear BVH (milliseconds on millions of triangles, more box tests per ray; csrc/pt_lbvh.hip); 'ploc': the
      // locally-ordered clustering of include/mi3pt.h (trees of the SAH class; csrc/pt_ploc.hip).  Also the rebuild a refit above
      // refitCostLimit falls back to, which is what makes a finite limit affordable: lastRefitMs then reports that build
      native.uploadTriangles(handle, packed.triangleBytes);
      const built = native.deviceBuildBvhEx(handle, flat.triangles.length, builder.method, builder.radius, builder.maxSearchIterations);
      nodeBytes = built.nodes;
      if (this.renderer.lastRefitCostRatio !== null) this.renderer.lastRefitMs = built.ms;
      this.lastDeviceBuild = { ms: built.ms, searchIterations: built.searchIterations, forcedIterations: built.forcedIterations };
      native.uploadBvh(handle, nodeBytes);
      this.builtNodeBytes = nodeBytes;
    } else {
      nodeBytes = native.hostBuildBvhF64(packed.positions, this.renderer.options.builderThreads || 0);
      native.uploadBvh(handle, nodeBytes);
      native.uploadTriangles(handle, packed.triangleBytes);
      this.builtNodeBytes = nodeBytes;
    }
    this.nodeBytes = nodeBytes;          // the host's copy of the records the device holds
    native.uploadMaterials(handle, packed.materialBytes);
    scene.needsUpdate = false;
    this.renderer._sceneVersion++;
    this.renderer._trianglesUploaded = flat.triangles.length;      // (reprojectScene: the count the next scene must have)
    this.stats = { Triangles: flat.triangles.length, Materials: flat.materials.length, 'BVH Nodes': nodeBytes.length / 48 };
    if (this.renderer.options.verbose) console.table(this.stats);                     // raytrace.ts:528-532
  }

  // renderer.refit (no counterpart in the reference, which rebuilds on every scene.needsUpdate, raytrace.ts:380-533): when only vertices
  // moved -- the triangle count is the last upload's and a tree is uploaded -- the triangles go up first, the device re-fits the boxes of
  // the uploaded tree to them (mi3pt_device_refit_bvh: the exact boxes of the old topology) and the host uploads those records.  The
  // price is tree quality: mi3pt_host_bvh_cost of the result over that of the last full build is renderer.lastRefitCostRatio; above
  // renderer.refitCostLimit (default Infinity: never) the caller rebuilds as it always did.  Returns the uploaded records, or null
  // when the caller has to build (lastRefitCostRatio then says why: null = no refit was possible).
  refitScene(packed, count) {
    const r = this.renderer, native = r.native, handle = r.handle;
    r.lastRefitCostRatio = null;
    r.lastRefitMs = null;
    if (!this.nodeBytes || !this.builtNodeBytes || count !== r._trianglesUploaded) return null;
    native.uploadTriangles(handle, packed.triangleBytes);
    const refitted = native.deviceRefitBvh(handle, this.nodeBytes.length / 48);
    if (this.builtCost === undefined || this.builtCostOf !== this.builtNodeBytes) {
      this.builtCost = native.hostBvhCost(this.builtNodeBytes);
      this.builtCostOf = this.builtNodeBytes;
    }
    const cost = native.hostBvhCost(refitted.nodes);
    r.lastRefitMs = refitted.ms;
    r.lastRefitCostRatio = this.builtCost > 0 ? cost / this.builtCost : (cost > 0 ? Infinity : 1);
    if (r.lastRefitCostRatio > r.refitCostLimit) return null;
    native.uploadBvh(handle, refitted.nodes);
    return refitted.nodes;
  }

  render(commandEncoder) { commandEncoder.passes |= SUBMIT_RAYTRACE; }     // raytrace.ts:696-708
}
module.exports = { RaytracePass };
