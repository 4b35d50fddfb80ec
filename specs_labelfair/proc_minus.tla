------------------------------ MODULE proc_minus ------------------------------
(* Written to show: A `-` LABEL INSIDE A PROCEDURE: the fair Caller reaches park, whose conjunct is WF_vars((pc[0] \notin {"rest_p1"}) /\ ...): nothing obliges a step at `rest`.  Termination is VIOLATED by stuttering there; the Caller's own labels and the procedure's other label stay weakly fair. *)
EXTENDS Naturals

(* --algorithm proc_minus
variables x = 0;

procedure park()
begin
  in:    x := 1;
  rest:- x := 2;
         return;
end procedure

fair process Caller = 0
begin
  c: call park();
  d: x := 3;
end process

end algorithm *)

=============================================================================
