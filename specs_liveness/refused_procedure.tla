------------------------------ MODULE refused_procedure ------------------------------
(* A procedure: pcal2tla gives it fairness conjuncts of its own; Termination is not checked. *)
EXTENDS Naturals

(* --algorithm refused_procedure
variables x = 0;

procedure Bump()
begin
  B: x := x + 1;
     return;
end procedure

fair process P = 0
begin
  A: call Bump();
end process

end algorithm *)
=============================================================================
